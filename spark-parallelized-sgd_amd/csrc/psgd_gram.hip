// psgd_gram.hip -- the second-moment pass over the registered partitions (psgd_gramian): with
// z_i = [x_i0 .. x_i,d-1, y_i, 1] (a = d + 2 columns) it returns M = sum_i z_i z_i^T, a x a doubles,
// row-major, both triangles (the lower an exact copy of the upper). X^T X = M[:d, :d], X^T y =
// M[:d, d], y^T y = M[d, d], the column sums M[:d, d + 1], sum y = M[d, d + 1], the row count
// M[d + 1, d + 1]. All arithmetic is fp64 whatever the storage. With a weight per row
// (psgd_gramian_weighted) the same kernels return M_w = sum_i w_i z_i z_i^T in the same layout: the
// Hessian of a loss sum when w is the rows' curvature (psgd_hessian.hip), weighted least squares' moments
// when w are instance weights.
//
// The tiling is the statistics passes' (tile0[p] is partition p's first tile, numbered across the
// partitions in partition-index order), as in psgd_grad.hip.
//
// Dense rows, v_mfma_f64_16x16x4_f64, bitwise reproducible. M is cut into 16-column blocks
// (nb = ceil(a / 16)); lane l of a fragment F(c0) of rows i0 .. i0 + 4 holds z[i0 + (l >> 4)][c0 + (l & 15)],
// which is the A operand (A[m = l & 15][k = l >> 4]) of block row c0 and the B operand
// (B[k = l >> 4][n = l & 15]) of block column c0 at once: M[j0.., k0..] += mfma(F(j0), F(k0)) with no
// transposition. A work item is (row span, tile group): a span is a run of consecutive tiles, a group a
// rectangle of gr x gc blocks, and only the groups that meet the upper triangle are kept
// (gram_groups). One wave keeps a group's accumulators (4 doubles a lane a block) in registers for
// the whole span, steps through it 4 rows at a time and ends with one record; gram_merge adds the
// records in span order and mirrors into the lower triangle. The four waves of a workgroup take four
// consecutive items, that is four groups of one span: they walk the same rows at the same pace and
// the rows' lines are shared through L2 (DESIGN.md section 3 counts the bytes). No floating-point
// atomics; the summation order is fixed by the tiling and the plan (gram_geometry), never by the
// grid: the same bits from call to call.
// Masking is by selection: a fragment lane at a column >= d loads feature d - 1 instead (a zero-copy
// row's pad columns may hold NaN and are never read) and takes the label, 1.0 or 0.0; a lane at a row
// past its tile's end loads the tile's last row and takes 0.0. Nothing loaded is multiplied away.
//
// CSR rows, one pass, NOT bitwise reproducible but for the three scalars: a row's entries with its
// label at column d and 1.0 at column d + 1 form an outer product whose upper triangle (columns
// increase within a row, so pair p <= q lands at M[col_p][col_q]) is added into M with fp64 vector
// atomics. y^T y, sum y and the count are per-tile sums merged in tile order (grad_merge_records);
// gram_mirror places them and copies the upper triangle into the lower.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "psgd_device.h"
#include "psgd_eval.h"

namespace psgd {
namespace {

constexpr int kGramBlock = 256;
constexpr int kGramWaves = kGramBlock / 64;
constexpr int kGramSub = 2;              // 4-row steps whose fragments are loaded together (one stage)
constexpr int64_t kGramItems = 2048;     // items the plan aims at: two rounds of one wave a SIMD
typedef double gram_d4 __attribute__((ext_vector_type(4)));

// First kept group of group row R: the first whose last block column reaches the row's first block.
__host__ __device__ inline int gram_first_group(int R, int gr, int gc) { return R * gr / gc; }

// W: the row-weighted pass M_w = sum_i w_i z_i z_i^T. omega holds one double per registered row in
// local row order, row0[p] is partition p's first row in it. The weight of a fragment's row comes
// with its label and multiplies the A operand alone (a[r] = valid ? v * w : 0.0; b[c] is z as it
// is): one v_mul_f64 per row fragment and sub-step, one rounding of z * w before the MFMA's exact
// products are added. Groups, spans, records and the order of every sum are the unweighted pass's, so
// omega == 1.0 everywhere gives its bits.
// The weights are a trailing parameter pack (none, or one GramOmega) so that the unweighted kernel's
// arguments, and with them its code, are what they were.
struct GramOmega {
    const double* omega;
    const int64_t* row0;
};
template <typename S, int GR, int GC, typename... Om>
__global__ __launch_bounds__(kGramBlock, 1) void gram_dense(const ChainDesc* __restrict__ descs,
                                                           const int64_t* __restrict__ tile0, int P,
                                                           int64_t n_tiles, GramGeom gm, double* __restrict__ rec,
                                                           Om... om) {
    constexpr bool W = sizeof...(Om) == 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t item = (int64_t)blockIdx.x * kGramWaves + wave;
    if (item >= gm.n_spans * gm.n_groups) return;
    const int64_t span = item / gm.n_groups;
    int left = (int)(item - span * gm.n_groups);
    int R = 0;
    for (;; ++R) {
        const int n = gm.ncg - gram_first_group(R, GR, GC);
        if (left < n) break;
        left -= n;
    }
    const int C = gram_first_group(R, GR, GC) + left;
    const int jb0 = R * GR, kb0 = C * GC;
    const int d = gm.d;
    // block (r, c) of the group is computed when it lies in the upper triangle and inside M
    unsigned on = 0;
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c)
            if (jb0 + r <= kb0 + c && kb0 + c < gm.nb) on |= 1u << (r * GC + c);
    on = __builtin_amdgcn_readfirstlane(on);
    const int m = lane & 15, kq = lane >> 4;
    // the lane's column of each fragment, and the feature column it loads: a lane at a column >= d
    // loads feature d - 1 instead (in bounds, never a pad column) and its value is not used
    int ca[GR], cb[GC], la[GR], lb[GC];
#pragma unroll
    for (int r = 0; r < GR; ++r) {
        ca[r] = (jb0 + r) * 16 + m;
        la[r] = ca[r] < d ? ca[r] : d - 1;
    }
#pragma unroll
    for (int c = 0; c < GC; ++c) {
        cb[c] = (kb0 + c) * 16 + m;
        lb[c] = cb[c] < d ? cb[c] : d - 1;
    }
    // fragments whose 16 columns are all features (all but the one or two that hold the label, the ones
    // column and the padding): bits 0 .. GR - 1 the row fragments, GR .. GR + GC - 1 the column fragments
    unsigned pure = 0;
#pragma unroll
    for (int r = 0; r < GR; ++r)
        if ((jb0 + r) * 16 + 16 <= d) pure |= 1u << r;
#pragma unroll
    for (int c = 0; c < GC; ++c)
        if ((kb0 + c) * 16 + 16 <= d) pure |= 1u << (GR + c);
    pure = __builtin_amdgcn_readfirstlane(pure);
    gram_d4 acc[GR][GC];
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c) acc[r][c] = gram_d4{0.0, 0.0, 0.0, 0.0};

    const int64_t t0 = span * gm.span;
    const int64_t t1 = t0 + gm.span < n_tiles ? t0 + gm.span : n_tiles;
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        if (r1 <= r0) continue;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        const double* orow = nullptr;
        if constexpr (W) {
            const GramOmega go = (om, ...);
            orow = go.omega + go.row0[p];
        }
        // A stage's loads carry no branch and no conversion, so that they stay in flight under the
        // MFMAs of the stage before: a row past the tile's end loads the tile's last row, a column
        // >= d feature d - 1 (plain loads: the other groups' waves of this span read the same
        // lines from L2), and the label comes with every sub-step. z[row][col] is selected from
        // them at its use: nothing loaded at a column >= d or a row >= r1 reaches an MFMA.
        auto load = [&](S (&fa)[kGramSub][GR], S (&fb)[kGramSub][GC], double (&fy)[kGramSub],
                        double (&fo)[kGramSub], int64_t rb) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < kGramSub; ++s) {
                const int64_t row = rb + 4 * s + kq;
                const int64_t rr = row < r1 ? row : r1 - 1;
                const gptr<S> xr = as_global(X + rr * dsc.ld);   // (global, not flat: the waits count loads)
#pragma unroll
                for (int r = 0; r < GR; ++r) fa[s][r] = xr[la[r]];
#pragma unroll
                for (int c = 0; c < GC; ++c) fb[s][c] = xr[lb[c]];
                fy[s] = as_global(dsc.y)[rr];
                if constexpr (W) fo[s] = as_global(orow)[rr];
            }
        };
        // (a fragment of features alone takes one select; the lane tests of the others are made where
        // they are used: kept over the loop as lane masks they spill the scalar registers)
        auto select = [&](S x, double y, int col, bool valid, bool all_features) __attribute__((always_inline)) -> double {
            double v = (double)x;
            if (!all_features) {
                int dl = d;
                asm volatile("" : "+s"(dl));
                v = col < dl ? v : col == dl ? y : col == dl + 1 ? 1.0 : 0.0;
            }
            return valid ? v : 0.0;
        };
        // (the weighted A operand: the selected z times the row's weight, then the row mask -- a row
        // past the tile's end gives 0.0 by selection, whatever weight was loaded for it)
        auto select_w = [&](S x, double y, double o, int col, bool valid, bool all_features) __attribute__((always_inline)) -> double {
            const double v = select(x, y, col, true, all_features) * o;
            return valid ? v : 0.0;
        };
        auto compute = [&](const S (&fa)[kGramSub][GR], const S (&fb)[kGramSub][GC], const double (&fy)[kGramSub],
                           const double (&fo)[kGramSub], int64_t rb) __attribute__((always_inline)) {
            // (the masks are re-read here as scalars: hoisted out of the loop their tests are kept as
            // lane masks, one each, and spill the scalar registers)
            unsigned onl = __builtin_amdgcn_readfirstlane(on);
            asm volatile("" : "+s"(onl));
            unsigned pl = __builtin_amdgcn_readfirstlane(pure);
            asm volatile("" : "+s"(pl));
#pragma unroll
            for (int s = 0; s < kGramSub; ++s) {
                const bool valid = rb + 4 * s + kq < r1;
                double a[GR], b[GC];
#pragma unroll
                for (int r = 0; r < GR; ++r) {
                    if constexpr (W) a[r] = select_w(fa[s][r], fy[s], fo[s], ca[r], valid, (pl >> r) & 1u);
                    else a[r] = select(fa[s][r], fy[s], ca[r], valid, (pl >> r) & 1u);
                }
#pragma unroll
                for (int c = 0; c < GC; ++c) b[c] = select(fb[s][c], fy[s], cb[c], valid, (pl >> (GR + c)) & 1u);
#pragma unroll
                for (int r = 0; r < GR; ++r)
#pragma unroll
                    for (int c = 0; c < GC; ++c)
                        if ((onl >> (r * GC + c)) & 1u)
                            acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[c], acc[r][c], 0, 0, 0);
            }
        };
        // two sets of fragments: the next stage's loads are in flight under this stage's MFMAs (the
        // loads past the tile's end re-read its last row and are dropped)
        constexpr int64_t stage = 4 * kGramSub;
        S xa[kGramSub][GR], xb[kGramSub][GC], ya[kGramSub][GR], yb[kGramSub][GC];
        double xy[kGramSub], yy[kGramSub];
        double xo[kGramSub], yo[kGramSub];   // (W only: dead, and gone, in the unweighted kernel)
        int64_t rb = r0;
        load(xa, xb, xy, xo, rb);
        while (rb < r1) {
            load(ya, yb, yy, yo, rb + stage);
            compute(xa, xb, xy, xo, rb);
            rb += stage;
            if (rb >= r1) break;
            load(xa, xb, xy, xo, rb + stage);
            compute(ya, yb, yy, yo, rb);
            rb += stage;
        }
    }
    // block (r, c)'s 256 doubles lie row-major: reg * 64 + lane = 16 * ((lane >> 4) + 4 reg) + (lane & 15)
    double* out = rec + item * ((int64_t)GR * GC * 256);
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c)
            if ((on >> (r * GC + c)) & 1u) {
#pragma unroll
                for (int q = 0; q < 4; ++q) out[((r * GC + c) * 4 + q) * 64 + lane] = acc[r][c][q];
            }
}

// Thread (j, k), j <= k: the spans' records of M[j][k] added in span order, written to both triangles.
__global__ __launch_bounds__(kGramBlock) void gram_merge(const double* __restrict__ rec, GramGeom gm,
                                                         double* __restrict__ out) {
    const int k = blockIdx.x * kGramBlock + threadIdx.x;
    const int j = blockIdx.y;
    if (k >= gm.a || j > k) return;
    const int jb = j >> 4, kb = k >> 4;
    const int R = jb / gm.gr, C = kb / gm.gc;
    int g = C - gram_first_group(R, gm.gr, gm.gc);
    for (int q = 0; q < R; ++q) g += gm.ncg - gram_first_group(q, gm.gr, gm.gc);
    const int64_t recsz = (int64_t)gm.gr * gm.gc * 256;
    const double* src = rec + g * recsz + (int64_t)((jb - R * gm.gr) * gm.gc + (kb - C * gm.gc)) * 256 +
                        (j & 15) * 16 + (k & 15);
    double s = 0.0;
    for (int64_t sp = 0; sp < gm.n_spans; ++sp) s += src[sp * gm.n_groups * recsz];
    out[(int64_t)j * gm.a + k] = s;
    out[(int64_t)k * gm.a + j] = s;
}

// ---- CSR ----
// W: every outer product is scaled by its row's weight (vp takes it) and the three scalars become
// sum w y^2, sum w y and sum w.
template <typename S, typename... Om>
__global__ __launch_bounds__(kGramBlock) void gram_csr(const ChainDesc* __restrict__ descs,
                                                       const int64_t* __restrict__ tile0, int P, int64_t n_tiles,
                                                       GramGeom gm, double* out, double* __restrict__ rec, Om... om) {
    constexpr bool W = sizeof...(Om) == 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gl = gm.group, rpw = 64 / gl;
    const int g = lane / gl, j = lane & (gl - 1);
    const int d = gm.d;
    const int64_t a = gm.a;
    for (int64_t tile = (int64_t)blockIdx.x * kGramWaves + wave; tile < n_tiles;
         tile += (int64_t)gridDim.x * kGramWaves) {
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        const S* val = reinterpret_cast<const S*>(dsc.x);
        double yy = 0.0, sy = 0.0, cnt = 0.0;
        for (int64_t rb = r0; rb < r1; rb += rpw) {
            const int64_t r = rb + g;
            if (r < r1) {
                const int64_t b = dsc.row_ptr[r];
                const int n = (int)(dsc.row_ptr[r + 1] - b);
                const double y = dsc.y[r];
                double o = 1.0;
                if constexpr (W) {
                    const GramOmega go = (om, ...);
                    o = go.omega[go.row0[p] + r];
                }
                // entry p against entries p .., the label (q = n) and the ones column (q = n + 1)
                for (int pi = 0; pi < n; ++pi) {
                    double vp = (double)val[b + pi];
                    if constexpr (W) vp = vp * o;
                    double* row = out + (int64_t)dsc.col[b + pi] * a;
                    for (int q = pi + j; q < n + 2; q += gl) {
                        const int cq = q < n ? dsc.col[b + q] : d + (q - n);
                        const double vq = q < n ? (double)val[b + q] : q == n ? y : 1.0;
                        unsafeAtomicAdd(row + cq, vp * vq);
                    }
                }
                if (j == 0) {
                    if constexpr (W) {
                        const double oy = o * y;
                        yy += oy * y;
                        sy += oy;
                        cnt += o;
                    } else {
                        yy += y * y;
                        sy += y;
                        cnt += 1.0;
                    }
                }
            }
        }
        yy = wave_sum(yy);
        sy = wave_sum(sy);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            rec[3 * tile] = yy;
            rec[3 * tile + 1] = sy;
            rec[3 * tile + 2] = cnt;
        }
    }
}

// Thread (j, k), j <= k: M[k][j] = M[j][k]; the three entries of the label and ones columns against
// each other come from sc = {y^T y, sum y, count}.
__global__ __launch_bounds__(kGramBlock) void gram_mirror(double* out, int d, const double* __restrict__ sc) {
    const int a = d + 2;
    const int k = blockIdx.x * kGramBlock + threadIdx.x;
    const int j = blockIdx.y;
    if (k >= a || j > k) return;
    double v = out[(int64_t)j * a + k];
    if (j >= d) {
        v = j == d ? (k == d ? sc[0] : sc[1]) : sc[2];
        out[(int64_t)j * a + k] = v;
    }
    out[(int64_t)k * a + j] = v;
}

// Back-to-back v_mfma_f64_16x16x4_f64 on `chains` independent accumulators a wave: the issue rate.
// The instruction is written out with its accumulators where they live over the back edge, in VGPRs
// (through the builtin they were copied into AGPRs and back around every MFMA), so the loop body is
// MFMAs and the counter alone. One chain is a dependent chain: C is the D of the MFMA before. The launch reserves kMfmaRateLds of LDS: one workgroup a CU, one wave a SIMD.
constexpr int kMfmaRateLds = 96 * 1024;
template <int CHAINS>
__global__ __launch_bounds__(kGramBlock, 1) void mfma_rate(int iters, double* out) {
    gram_d4 acc[CHAINS];
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) acc[c] = gram_d4{0.0, 0.0, 0.0, 0.0};
    const double x = (double)(threadIdx.x & 7) * 0.125, y = (double)(threadIdx.x & 3) * 0.25;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int c = 0; c < CHAINS; ++c)
            asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(acc[c]) : "v"(x), "v"(y));
    }
    // (the compiler does not see an MFMA in the asm: the last results land before they are read)
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc[c]));
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
    if (s == -1.0) out[0] = s;   // (never true: the sums are >= 0; keeps the loop alive)
}

template <int CHAINS>
int launch_mfma_rate(int blocks, int iters, double* out, hipStream_t st) {
    auto k = mfma_rate<CHAINS>;
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, kMfmaRateLds);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kGramBlock), kMfmaRateLds, st, iters, out);
    return (int)hipGetLastError();
}

template <typename S>
int launch_dense_s(const GramGeom& gm, hipStream_t st, const ChainDesc* descs, const int64_t* tile0, int P,
                   int64_t n_tiles, double* rec, const double* omega, const int64_t* row0) {
    const int64_t items = gm.n_spans * gm.n_groups;
    const dim3 gr((unsigned)((items + kGramWaves - 1) / kGramWaves)), bl(kGramBlock);
    if (omega) {
        const GramOmega go{omega, row0};
        if (gm.gr == 1 && gm.gc == 1)
            hipLaunchKernelGGL((gram_dense<S, 1, 1, GramOmega>), gr, bl, 0, st, descs, tile0, P, n_tiles, gm, rec, go);
        else if (gm.gr == 1 && gm.gc == 2)
            hipLaunchKernelGGL((gram_dense<S, 1, 2, GramOmega>), gr, bl, 0, st, descs, tile0, P, n_tiles, gm, rec, go);
        else if (gm.gr == 2 && gm.gc == 4)
            hipLaunchKernelGGL((gram_dense<S, 2, 4, GramOmega>), gr, bl, 0, st, descs, tile0, P, n_tiles, gm, rec, go);
        else if (gm.gr == 4 && gm.gc == 8)
            hipLaunchKernelGGL((gram_dense<S, 4, 8, GramOmega>), gr, bl, 0, st, descs, tile0, P, n_tiles, gm, rec, go);
        else
            return (int)hipErrorInvalidValue;
        return (int)hipGetLastError();
    }
    if (gm.gr == 1 && gm.gc == 1)
        hipLaunchKernelGGL((gram_dense<S, 1, 1>), gr, bl, 0, st, descs, tile0, P, n_tiles, gm, rec);
    else if (gm.gr == 1 && gm.gc == 2)
        hipLaunchKernelGGL((gram_dense<S, 1, 2>), gr, bl, 0, st, descs, tile0, P, n_tiles, gm, rec);
    else if (gm.gr == 2 && gm.gc == 4)
        hipLaunchKernelGGL((gram_dense<S, 2, 4>), gr, bl, 0, st, descs, tile0, P, n_tiles, gm, rec);
    else if (gm.gr == 4 && gm.gc == 8)
        hipLaunchKernelGGL((gram_dense<S, 4, 8>), gr, bl, 0, st, descs, tile0, P, n_tiles, gm, rec);
    else
        return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

}  // namespace

int gram_groups(int nb, int gr, int gc) {
    const int nrg = (nb + gr - 1) / gr, ncg = (nb + gc - 1) / gc;
    int n = 0;
    for (int R = 0; R < nrg; ++R) n += ncg - gram_first_group(R, gr, gc);
    return n;
}

GramGeom gram_geometry(int layout, int storage, int d, int64_t n_tiles, int64_t max_nnz) {
    GramGeom gm{};
    gm.d = d;
    gm.a = d + 2;
    gm.nb = (gm.a + 15) / 16;
    gm.tile_rows = stats_geometry(layout, d, storage).tile_rows;
    if (layout == kCsr) {
        gm.path = 1;
        const int64_t len = max_nnz + 2;   // a row's entries with its label and the ones column
        gm.group = len <= 16 ? 16 : len <= 32 ? 32 : 64;
        gm.span = grad_merge_span(n_tiles > 0 ? n_tiles : 1);
        gm.n_spans = n_tiles > 0 ? (n_tiles + gm.span - 1) / gm.span : 0;
        gm.scratch_bytes = n_tiles > 0 ? (n_tiles + gm.n_spans + 1) * 3 * (int64_t)sizeof(double) : 0;
        return gm;
    }
    // the smallest built rectangle that holds M's blocks, 4 x 8 (256 accumulator registers) at most
    if (gm.nb == 1) { gm.gr = 1; gm.gc = 1; }
    else if (gm.nb == 2) { gm.gr = 1; gm.gc = 2; }
    else if (gm.nb <= 8) { gm.gr = 2; gm.gc = 4; }
    else { gm.gr = 4; gm.gc = 8; }
    gm.nrg = (gm.nb + gm.gr - 1) / gm.gr;
    gm.ncg = (gm.nb + gm.gc - 1) / gm.gc;
    gm.n_groups = gram_groups(gm.nb, gm.gr, gm.gc);
    if (n_tiles <= 0) {
        gm.span = 1;
        return gm;
    }
    // a narrow d takes its parallelism from spans, a wide d from groups: about kGramItems items of
    // 4 x 8 blocks, more of the smaller rectangles (their waves are several a SIMD and wait on loads)
    const int64_t items = kGramItems * (gm.gr * gm.gc >= 32 ? 1 : gm.gr * gm.gc >= 8 ? 2 : 4);
    int64_t want = (items + gm.n_groups - 1) / gm.n_groups;
    if (want > n_tiles) want = n_tiles;
    gm.span = (n_tiles + want - 1) / want;
    gm.n_spans = (n_tiles + gm.span - 1) / gm.span;
    gm.scratch_bytes = gm.n_spans * gm.n_groups * gm.gr * gm.gc * 256 * (int64_t)sizeof(double);
    return gm;
}

int launch_gramian_dense(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                         const GramGeom& gm, int storage, double* rec, double* out, hipStream_t st,
                         const double* omega, const int64_t* row0) {
    if (n_tiles <= 0) return (int)hipMemsetAsync(out, 0, (size_t)gm.a * gm.a * sizeof(double), st);
    const int e = storage == 1 ? launch_dense_s<float>(gm, st, descs, tile0, n_parts, n_tiles, rec, omega, row0)
                               : launch_dense_s<double>(gm, st, descs, tile0, n_parts, n_tiles, rec, omega, row0);
    if (e) return e;
    hipLaunchKernelGGL(gram_merge, dim3((unsigned)((gm.a + kGramBlock - 1) / kGramBlock), (unsigned)gm.a),
                       dim3(kGramBlock), 0, st, rec, gm, out);
    return (int)hipGetLastError();
}

int launch_gramian_csr(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                       const GramGeom& gm, int storage, double* rec, double* out, int num_cus, hipStream_t st,
                       const double* omega, const int64_t* row0) {
    int e = (int)hipMemsetAsync(out, 0, (size_t)gm.a * gm.a * sizeof(double), st);
    if (e || n_tiles <= 0) return e;
    const unsigned blocks = grad_balanced_blocks(n_tiles, num_cus, 8);
    if (omega && storage == 1)
        hipLaunchKernelGGL((gram_csr<float, GramOmega>), dim3(blocks), dim3(kGramBlock), 0, st, descs, tile0, n_parts,
                           n_tiles, gm, out, rec, GramOmega{omega, row0});
    else if (omega)
        hipLaunchKernelGGL((gram_csr<double, GramOmega>), dim3(blocks), dim3(kGramBlock), 0, st, descs, tile0, n_parts,
                           n_tiles, gm, out, rec, GramOmega{omega, row0});
    else if (storage == 1)
        hipLaunchKernelGGL(gram_csr<float>, dim3(blocks), dim3(kGramBlock), 0, st, descs, tile0, n_parts, n_tiles, gm,
                           out, rec);
    else
        hipLaunchKernelGGL(gram_csr<double>, dim3(blocks), dim3(kGramBlock), 0, st, descs, tile0, n_parts, n_tiles, gm,
                           out, rec);
    e = (int)hipGetLastError();
    if (e) return e;
    // {y^T y, sum y, count}: the tiles' sums in tile order, behind the tiles' and spans' records
    double* rec2 = rec + 3 * n_tiles;
    double* sc = rec2 + 3 * gm.n_spans;
    e = grad_merge_records(rec, n_tiles, 3, rec2, sc, st);
    if (e) return e;
    hipLaunchKernelGGL(gram_mirror, dim3((unsigned)((gm.a + kGramBlock - 1) / kGramBlock), (unsigned)gm.a),
                       dim3(kGramBlock), 0, st, out, gm.d, sc);
    return (int)hipGetLastError();
}

}  // namespace psgd

extern "C" int32_t psgd_gram_mfma_rate(int32_t blocks, int32_t chains, int32_t iters, double* d_out, void* stream) {
    if (blocks <= 0 || iters <= 0 || !d_out) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (chains) {
        case 1: return psgd::launch_mfma_rate<1>(blocks, iters, d_out, st);
        case 2: return psgd::launch_mfma_rate<2>(blocks, iters, d_out, st);
        case 4: return psgd::launch_mfma_rate<4>(blocks, iters, d_out, st);
        case 8: return psgd::launch_mfma_rate<8>(blocks, iters, d_out, st);
    }
    return -1;
}
