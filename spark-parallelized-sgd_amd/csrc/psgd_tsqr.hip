// psgd_tsqr.hip -- the tall-skinny QR pass over the registered partitions (psgd_tsqr): with
// z_i = [x_i0 .. x_i,d-1, y_i] (a = d + 1 <= 128 columns) it returns the a x a upper-triangular R with
// R^T R = Z^T Z and a non-negative diagonal, computed by orthogonal transformations alone: Z^T Z is never
// formed, so R carries cond(Z), not its square. All arithmetic is fp64 whatever the storage.
//
// A work item is a span of consecutive tiles of the statistics passes' tiling (tsqr_geometry, host
// code). One workgroup of four waves takes an item. It keeps R in LDS, zero at first, as the
// nb (nb + 1) / 2 blocks of 16 x 16 doubles on and above the block diagonal (nb = ceil(a / 16)), and a
// panel P of T = 64 rows by a_pad = 16 nb columns. A panel is the next 64 rows of a tile, widened to
// f64 as they are stored into LDS, the label at column d, zeros at the pad columns and at the rows past
// the tile's end. Each panel is folded into R by the triangular-on-rectangular QR of [R; P] (LAPACK's
// dtpqrt with l = 0): the reflector of column j is [e_j; v_j], it touches row j of R and the rows of P.
// The work is blocked by 16 columns, the N of v_mfma_f64_16x16x4_f64. For block jb:
//   panel phase (wave 0, vector unit). Lane (g = l >> 4, k = l & 15) holds column k of the block: the
//     16 rows g + 4 i of P, column k of R's diagonal block, and row k of the triangular factor Tf of the
//     compact WY form. Column j: its norm is 16 fma a lane and two cross-row adds; the reflector as
//     dlarfg forms it (beta = -sign(alpha) ||[alpha; x]||, tau = (beta - alpha) / beta, v = x / (alpha -
//     beta); tau = 0 and H = I when x is zero, so a zero column leaves its diagonal as it is and nothing
//     divides by zero); v goes through LDS (V2t, transposed) to every lane; one dot product v . p_k a
//     lane then serves the columns right of j (w_k = R[j][k] + v . p_k; R[j][k] -= tau w_k; p_k -= tau
//     w_k v) and the columns left of it (v_k . v_j, the terms of Tf's column j, dtpqrt2's recurrence).
//   trailing update (all waves, matrix cores), the column blocks c > jb dealt over the waves:
//     W = R[jb, c] + V2^T P[:, c] (16 MFMAs, K = 64); W <- Tf^T W (4 MFMAs; W's accumulators are the B
//     operand as they stand); R[jb, c] -= W; P[:, c] -= V2 W (4 row chunks x 4 MFMAs, K = 16, V2 read
//     from its transposed copy).
// The columns at and past a (the last block's padding) are skipped by a wave-uniform test; they stay zero.
// LDS operands: P's pitch is a_pad rounded to 16 mod 32 doubles and V2t's is 80, so the four rows
// an MFMA operand touches (lane l reads [row0 + (l >> 4)][col0 + (l & 15)]) start 32 banks apart
// alternately: one ds_read_b64 a lane and operand, no two lanes of a half-wave on one bank.
// Barriers: one after a panel is stored, two a block (after its panel phase, after its trailing update).
// The next panel's global loads are issued before the first of them and land under the factorisation.
//
// An item ends by writing its R as a_pad rows of a_pad doubles into its scratch slot. The merge is this
// kernel again over those rows (f64, no label column): a node takes `fan` children in slot order, and
// writes into its first child's slot, so the scratch is the items' slots and nothing more. The tree is
// fixed by the plan: the same bits from call to call, no atomics. The last node flips the rows whose
// diagonal is negative and writes the a x a result.
#include "psgd_device.h"
#include "psgd_eval.h"

namespace psgd {
namespace {

constexpr int kTsqrBlock = 256;
constexpr int kTsqrPanel = 64;          // T: rows of a panel
constexpr int kTsqrVPitch = 80;         // V2t's pitch: 64 rows, 16 mod 32
constexpr int kTsqrMaxNb = 8;           // a <= 128
constexpr int kTsqrFan = 8;             // children of a merge node
constexpr int64_t kTsqrLds = 160 * 1024;
typedef double tsqr_d4 __attribute__((ext_vector_type(4)));

// Where an item's rows come from. Partitions: tiles [item span, (item + 1) span) of the registry.
struct TsqrParts {
    const ChainDesc* descs;
    const int64_t* tile0;
    int P;
    int tile_rows;
    int64_t n_tiles, span;
};
// Rows: chunks [item fan, (item + 1) fan) of a dense f64 array; chunk c is rows [c chunk_stride,
// c chunk_stride + chunk_rows) cut at n_rows.
struct TsqrRows {
    const double* base;
    int64_t n_rows, chunk_rows, chunk_stride, n_chunks, ld;
    int fan;
};
struct TsqrShape {
    int nfeat;      // columns a source row stores: d (the label comes from y), or a
    int a, nb;      // columns of Z, blocks of 16
    int pitch;      // P's pitch in LDS
};

__host__ __device__ inline int tsqr_blk(int rb, int cb, int nb) { return rb * nb - rb * (rb - 1) / 2 + (cb - rb); }

__global__ void tsqr_zero(double* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 0.0;
}

// LABEL: rows of the registered partitions (storage S, the label at column d); else f64 rows as they are.
// out + item * out_item_stride receives out_n rows of out_n doubles (out_n = a_pad, or a with `last`).
template <typename S, bool LABEL>
__global__ __launch_bounds__(kTsqrBlock, 1) void tsqr_dense(TsqrParts pt, TsqrRows rw, TsqrShape sh,
                                                           double* __restrict__ out, int64_t out_item_stride,
                                                           int out_n, int last) {
    extern __shared__ double tsqr_lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, k = lane & 15;
    const int nb = sh.nb, a = sh.a, pitch = sh.pitch, nfeat = sh.nfeat;
    double* const R = tsqr_lds;
    double* const Pn = R + (nb * (nb + 1) / 2) * 256;
    double* const Vt = Pn + kTsqrPanel * pitch;
    double* const Tf = Vt + 16 * kTsqrVPitch;
    const int64_t item = blockIdx.x;

    for (int f = tid; f < (nb * (nb + 1) / 2) * 256; f += kTsqrBlock) R[f] = 0.0;
    for (int f = tid; f < 16 * kTsqrVPitch; f += kTsqrBlock) Vt[f] = 0.0;

    // ---- the item's panels, in order: (X, Y, ld) the source of the current one, rows [pr0, r1) ----
    const S* X = nullptr;
    const double* Y = nullptr;
    int64_t ld = 0, rb = 0, r1 = 0, pr0 = 0;
    int64_t unit = LABEL ? item * pt.span : item * rw.fan;   // tile or chunk
    const int64_t unit_end = LABEL ? (unit + pt.span < pt.n_tiles ? unit + pt.span : pt.n_tiles)
                                   : (unit + rw.fan < rw.n_chunks ? unit + rw.fan : rw.n_chunks);
    auto next = [&]() -> bool {
        while (rb >= r1) {
            if (unit >= unit_end) return false;
            if constexpr (LABEL) {
                const int p = tile_partition(pt.tile0, pt.P, unit);
                const ChainDesc dsc = pt.descs[p];
                rb = (unit - pt.tile0[p]) * pt.tile_rows;
                r1 = rb + pt.tile_rows < dsc.n_rows ? rb + pt.tile_rows : dsc.n_rows;
                X = reinterpret_cast<const S*>(dsc.x);
                Y = dsc.y;
                ld = dsc.ld;
            } else {
                rb = unit * rw.chunk_stride;
                r1 = rb + rw.chunk_rows < rw.n_rows ? rb + rw.chunk_rows : rw.n_rows;
                X = reinterpret_cast<const S*>(rw.base);
                ld = rw.ld;
            }
            ++unit;
        }
        pr0 = rb;
        rb += kTsqrPanel;
        return true;
    };
    // A thread's part of a panel: rows (tid >> 4) + 16 i, i < 4, of column (tid & 15) of every block.
    // The loads carry no branch on the data: a row past the tile's end loads the tile's last row, a
    // column >= nfeat column nfeat - 1 (in bounds, never a pad column); both are dropped at the store.
    S xr[4 * kTsqrMaxNb];
    double yr[4];
    int nvalid = 0;
    const int lrow = tid >> 4;
    auto load = [&]() __attribute__((always_inline)) {
        nvalid = r1 - pr0 < kTsqrPanel ? (int)(r1 - pr0) : kTsqrPanel;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t row = pr0 + lrow + 16 * i;
            const int64_t rr = row < r1 ? row : r1 - 1;
            const gptr<S> src = as_global(X + rr * ld);
#pragma unroll
            for (int cb = 0; cb < kTsqrMaxNb; ++cb)
                if (cb < nb) {
                    const int col = cb * 16 + k;
                    xr[cb * 4 + i] = src[col < nfeat ? col : nfeat - 1];
                }
            if constexpr (LABEL) yr[i] = as_global(Y)[rr];
        }
    };
    auto store = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = lrow + 16 * i;
#pragma unroll
            for (int cb = 0; cb < kTsqrMaxNb; ++cb)
                if (cb < nb) {
                    const int col = cb * 16 + k;
                    double v = col < nfeat ? (double)xr[cb * 4 + i] : 0.0;
                    if constexpr (LABEL) v = col == nfeat ? yr[i] : v;
                    Pn[row * pitch + col] = row < nvalid ? v : 0.0;
                }
        }
    };

    bool have = next();
    if (have) load();
    while (have) {
        store();
        have = next();
        if (have) load();
        __syncthreads();
        for (int jb = 0; jb < nb; ++jb) {
            // ---- panel phase ----
            if (wave == 0) {
                double* const Rd = R + tsqr_blk(jb, jb, nb) * 256;
                double p[16], r[16], tr[16], v[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    p[i] = Pn[(g + 4 * i) * pitch + jb * 16 + k];
                    r[i] = Rd[i * 16 + k];
                    tr[i] = 0.0;
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if (jb * 16 + j < a) {   // (wave-uniform: the padding's columns are zero and stay so)
                        double t = 0.0;
#pragma unroll
                        for (int i = 0; i < 16; ++i) t = fma(p[i], p[i], t);
                        t = swap_sum32(swap_sum16(t));
                        const double ssq = readlane_d(t, j);
                        const double alpha = readlane_d(r[j], j);
                        const bool nz = ssq > 0.0;
                        const double nrm = sqrt(fma(alpha, alpha, ssq));
                        const double beta = alpha >= 0.0 ? -nrm : nrm;
                        const double tau = nz ? (beta - alpha) / beta : 0.0;
                        const double scale = nz ? 1.0 / (alpha - beta) : 0.0;
                        const double sc = k == j ? scale : 1.0;
#pragma unroll
                        for (int i = 0; i < 16; ++i) p[i] = p[i] * sc;
                        if (k == j) {
#pragma unroll
                            for (int i = 0; i < 16; ++i) Vt[j * kTsqrVPitch + 4 * i + g] = p[i];
                        }
                        wave_lds_sync();
                        double dot = 0.0;
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            v[i] = Vt[j * kTsqrVPitch + 4 * i + g];
                            dot = fma(v[i], p[i], dot);
                        }
                        dot = swap_sum32(swap_sum16(dot));
                        const double tw = k > j ? tau * (r[j] + dot) : 0.0;
                        r[j] = k == j ? (nz ? beta : alpha) : r[j] - tw;
#pragma unroll
                        for (int i = 0; i < 16; ++i) p[i] = fma(-tw, v[i], p[i]);
                        // Tf[:j, j] = -tau Tf[:j, :j] (V2[:, :j]^T v_j): lane k holds row k, z_m = v_m . v_j
                        const double z = k < j ? dot : 0.0;
                        double y = 0.0;
#pragma unroll
                        for (int m = 0; m < j; ++m) y = fma(tr[m], readlane_d(z, m), y);
                        tr[j] = k < j ? -tau * y : k == j ? tau : 0.0;
                    }
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) Pn[(g + 4 * i) * pitch + jb * 16 + k] = p[i];
                if (g == 0) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        Rd[i * 16 + k] = r[i];
                        Tf[k * 16 + i] = tr[i];
                    }
                }
            }
            __syncthreads();
            // ---- trailing update ----
            for (int c = jb + 1 + wave; c < nb; c += 4) {
                double* const Rb = R + tsqr_blk(jb, c, nb) * 256;
                tsqr_d4 r0, acc;
#pragma unroll
                for (int q = 0; q < 4; ++q) r0[q] = Rb[(4 * q + g) * 16 + k];
                acc = r0;
#pragma unroll
                for (int s = 0; s < kTsqrPanel / 4; ++s) {
                    const double* row = Pn + (4 * s + g) * pitch + k;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(row[jb * 16], row[c * 16], acc, 0, 0, 0);
                }
                tsqr_d4 w2 = tsqr_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    w2 = __builtin_amdgcn_mfma_f64_16x16x4f64(Tf[(4 * s + g) * 16 + k], acc[s], w2, 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) Rb[(4 * q + g) * 16 + k] = r0[q] - w2[q];
#pragma unroll
                for (int rc = 0; rc < kTsqrPanel / 16; ++rc) {
                    double* const Pc = Pn + (rc * 16 + g) * pitch + c * 16 + k;
                    tsqr_d4 pc;
#pragma unroll
                    for (int q = 0; q < 4; ++q) pc[q] = Pc[4 * q * pitch];
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        pc = __builtin_amdgcn_mfma_f64_16x16x4f64(Vt[(4 * s + g) * kTsqrVPitch + rc * 16 + k], -w2[s], pc,
                                                                  0, 0, 0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) Pc[4 * q * pitch] = pc[q];
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // ---- the item's R: upper triangle from the blocks, zeros below; the last node's diagonal >= 0 ----
    double* const dst = out + item * out_item_stride;
    for (int f = tid; f < out_n * out_n; f += kTsqrBlock) {
        const int row = f / out_n, col = f - row * out_n;
        double val = 0.0;
        if (row <= col) {
            val = R[tsqr_blk(row >> 4, col >> 4, nb) * 256 + (row & 15) * 16 + (col & 15)];
            if (last && R[tsqr_blk(row >> 4, row >> 4, nb) * 256 + (row & 15) * 17] < 0.0) val = -val;
        }
        dst[f] = val;
    }
}

template <typename S, bool LABEL>
int tsqr_launch(const TsqrGeom& gm, int64_t items, hipStream_t st, const TsqrParts& pt, const TsqrRows& rw, int nfeat,
                double* out, int64_t out_item_stride, int out_n, int last) {
    auto kern = tsqr_dense<S, LABEL>;
    if (gm.lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)gm.lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    const TsqrShape sh{nfeat, gm.a, gm.nb, gm.pitch};
    hipLaunchKernelGGL(kern, dim3((unsigned)items), dim3(kTsqrBlock), (size_t)gm.lds_bytes, st, pt, rw, sh, out,
                       out_item_stride, out_n, last);
    return (int)hipGetLastError();
}

int tsqr_zero_out(const TsqrGeom& gm, double* out, hipStream_t st) {
    const int n = gm.a * gm.a;
    hipLaunchKernelGGL(tsqr_zero, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out, n);
    return (int)hipGetLastError();
}

// The merge levels over the `items` slots of scratch the first level filled: level by level, a node
// into its first child's slot, the last one into out.
int tsqr_merge(const TsqrGeom& gm, double* scratch, double* out, hipStream_t st) {
    const int64_t slot = (int64_t)gm.a_pad * gm.a_pad;
    int64_t m = gm.items, stride = 1;
    while (m > 1) {
        const int64_t m2 = (m + gm.fan - 1) / gm.fan;
        const TsqrRows rw{scratch, gm.items * gm.a_pad, gm.a_pad, stride * gm.a_pad, m, gm.a_pad, gm.fan};
        const bool last = m2 == 1;
        const int e = tsqr_launch<double, false>(gm, m2, st, TsqrParts{}, rw, gm.a, last ? out : scratch,
                                                 last ? 0 : stride * gm.fan * slot, last ? gm.a : gm.a_pad, last);
        if (e) return e;
        m = m2;
        stride *= gm.fan;
    }
    return 0;
}

void tsqr_shape(TsqrGeom& gm, int a) {
    gm.a = a;
    gm.nb = (a + 15) / 16;
    gm.a_pad = 16 * gm.nb;
    gm.pitch = gm.a_pad % 32 == 16 ? gm.a_pad : gm.a_pad + 16;
    gm.panel_rows = kTsqrPanel;
    gm.fan = kTsqrFan;
    gm.lds_bytes = ((int64_t)(gm.nb * (gm.nb + 1) / 2) * 256 + (int64_t)kTsqrPanel * gm.pitch + 16 * kTsqrVPitch + 256) *
                   (int64_t)sizeof(double);
}

void tsqr_tree(TsqrGeom& gm) {
    gm.levels = 0;
    for (int64_t m = gm.items; m > 1; m = (m + gm.fan - 1) / gm.fan) ++gm.levels;
    gm.scratch_bytes = gm.items * gm.a_pad * gm.a_pad * (int64_t)sizeof(double);
}

}  // namespace

TsqrGeom tsqr_geometry(int storage, int d, int64_t n_tiles) {
    TsqrGeom gm{};
    gm.d = d;
    tsqr_shape(gm, d + 1);
    gm.tile_rows = stats_geometry(kDense, d, storage).tile_rows;
    gm.span = 1;
    if (n_tiles > 0) {
        // one workgroup a CU at the widest a, several at a narrow one: more items there
        int64_t want = gm.nb <= 2 ? 2048 : gm.nb <= 4 ? 1024 : 512;
        if (want > n_tiles) want = n_tiles;
        gm.span = (n_tiles + want - 1) / want;
        gm.items = (n_tiles + gm.span - 1) / gm.span;
    }
    tsqr_tree(gm);
    return gm;
}

TsqrGeom tsqr_rows_geometry(int a, int64_t n_rows) {
    TsqrGeom gm{};
    gm.d = a;
    tsqr_shape(gm, a);
    gm.tile_rows = gm.fan * gm.a_pad;   // a first-level item takes as many rows as a merge node
    gm.span = 1;
    gm.items = n_rows > 0 ? (n_rows + gm.tile_rows - 1) / gm.tile_rows : 0;
    tsqr_tree(gm);
    return gm;
}

int launch_tsqr(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles, const TsqrGeom& gm,
                int storage, double* scratch, double* out, hipStream_t st) {
    if (gm.lds_bytes > kTsqrLds) return (int)hipErrorInvalidValue;
    if (gm.items <= 0) return tsqr_zero_out(gm, out, st);
    const TsqrParts pt{descs, tile0, n_parts, gm.tile_rows, n_tiles, gm.span};
    const bool last = gm.items == 1;
    double* dst = last ? out : scratch;
    const int64_t stride = last ? 0 : (int64_t)gm.a_pad * gm.a_pad;
    const int n = last ? gm.a : gm.a_pad;
    const int e = storage == 1 ? tsqr_launch<float, true>(gm, gm.items, st, pt, TsqrRows{}, gm.d, dst, stride, n, last)
                               : tsqr_launch<double, true>(gm, gm.items, st, pt, TsqrRows{}, gm.d, dst, stride, n, last);
    return e ? e : tsqr_merge(gm, scratch, out, st);
}

int launch_tsqr_rows(const double* rows, int64_t n_rows, const TsqrGeom& gm, double* scratch, double* out,
                     hipStream_t st) {
    if (gm.lds_bytes > kTsqrLds) return (int)hipErrorInvalidValue;
    if (gm.items <= 0) return tsqr_zero_out(gm, out, st);
    const TsqrRows rw{rows, n_rows, gm.tile_rows, gm.tile_rows, gm.items, gm.a, 1};
    const bool last = gm.items == 1;
    const int e = tsqr_launch<double, false>(gm, gm.items, st, TsqrParts{}, rw, gm.a, last ? out : scratch,
                                             last ? 0 : (int64_t)gm.a_pad * gm.a_pad, last ? gm.a : gm.a_pad, last);
    return e ? e : tsqr_merge(gm, scratch, out, st);
}

}  // namespace psgd
