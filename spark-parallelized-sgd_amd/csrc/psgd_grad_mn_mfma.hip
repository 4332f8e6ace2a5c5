// psgd_grad_mn_mfma.hip -- the batch gradient of the multinomial LogisticGradient on the fp64 matrix
// cores (method PSGD_MN_METHOD_MFMA of psgd_gradient_sum_multinomial_method): dense rows, C1 = K - 1 <=
// 64 classes beside the pivot, d <= 4,096. The per-row math, the output {gradientSum[c d + j], lossSum,
// count}, the tiling, the sampled-batch convention (ChainDesc::rows) and the {loss, count} record a tile
// are psgd_grad_mn.hip's; so are the ranges of tiles whose multipliers the scratch holds at a time and
// the merge of the records (grad_merge_records). All arithmetic is fp64 whatever the storage; no
// floating-point atomics: the same bits from call to call, and the range changes none of them.
//
// grad_mn_pack_w writes W^T (d x C1) once a call into project_pack_b's operand order: index ((s nb + b)
// VEC + e) 64 + l holds W[16 b + (l & 15)][(4 s + (l >> 4)) VEC + e], zero past d or C1 -- dpad x 16 nb
// doubles, nb = ceil(C1 / 16) <= 4 class blocks, dpad = d rounded up to 4 row vectors. The multiplier
// pass reads it from LDS while it fits a CU's 160 KiB, else through L2, one 512-byte line an MFMA.
//
// Pass 1, grad_mn_rowmult_mfma: v_mfma_f64_16x16x4_f64 with M = rows, K = features, N = classes, in
// project_dense's geometry. A wave takes a tile, 16 batch rows at a time. Lane l = (m = l & 15, q = l >>
// 4) reads row m as 16-byte vectors at the row's own pitch (a sampled batch: rows[] once a group) and
// walks the features once with all nb class blocks in accumulators: the rows come from HBM once and the
// margins never leave registers. Loads carry no lane-conditional branch: a vector past the row's last
// reloads the last, a row past the tile's end the partition's last row; a feature >= d (a zero-copy
// row's pad may hold NaN) is replaced by 0.0 by selection, never multiplied away. After the walk the
// lane holds D[row = q + 4 reg][class = 16 b + m]. Per row: the maximum over the lane's blocks in
// ascending order with strict >, then over the 16 lanes of the DPP row as (value, index) pairs, the
// lower index winning an equal value (kmeans_assign_dense's argmin with the comparison turned; pad
// classes are -Inf by selection); every lane's own exponentials; their sum over the DPP row in a fixed
// order (exp(-M) in the maximum's place when M > 0); one division a (row, class); the indicator from
// the row's label; the row's margin at its label fetched by a sum of selections. Multipliers go to
// mult[(tile-local row) C1 + c], 0.0 for a row past the batch's end. The rows' losses are added in row
// order into the tile's record.
//
// Pass 2, grad_mn_wsum_mfma: the same instruction with M = classes, N = features, K = rows --
// kmeans_sums_dense with the A operand replaced. For rows i0 .. i0 + 3 the B operand is the fragment
// z[i0 + (l >> 4)][16 fb + (l & 15)] of the rows as they lie (a column >= d loads feature d - 1 and is
// zeroed by selection); the A operand is A[m][q] = mult[i0 + q][16 cb + m], 0.0 past C1 or past the
// tile's end, by selection. A wave keeps a rectangle of gr x gc blocks (class blocks x feature blocks,
// gr = 1, 2, 4 >= nb, gc = 2 or 8: 256 accumulator registers at most) over a piece of min(span, range)
// tiles, walked tile by tile, four rows a step; an item is (piece, rectangle). A record covers span = gr
// tiles (C1 d doubles, row-major: at most 3.2 % of the rows' bytes); an item that does not start its
// span continues from the span's record, so a range shorter than a span changes no operation and no
// bit. The records are merged in span order.
#include <algorithm>

#include "psgd_device.h"
#include "psgd_eval.h"

namespace psgd {
namespace {

constexpr int kMmBlock = 512;               // the multiplier pass
constexpr int kMmWaves = kMmBlock / 64;
constexpr int kMmU = 4;                     // steps whose vectors are loaded together (one stage)
constexpr int64_t kMmLds = 160 * 1024;      // a CU's LDS
constexpr int kMmSumBlock = 256;            // the accumulation pass
constexpr int kMmSumWaves = kMmSumBlock / 64;
constexpr int kMmSub = 2;                   // 4-row steps whose fragments are loaded together (one stage)
typedef double mm_d4 __attribute__((ext_vector_type(4)));

// Wp[((s nb + b) VEC + e) 64 + l] = W[16 b + (l & 15)][(4 s + (l >> 4)) VEC + e], zero past d or C1.
__global__ __launch_bounds__(256) void grad_mn_pack_w(const double* __restrict__ W, int d, int C1, int nb, int vec,
                                                      int64_t total, double* __restrict__ Wp) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int l = (int)(i & 63);
        int64_t t = i >> 6;
        const int e = (int)(t % vec);
        t /= vec;
        const int b = (int)(t % nb);
        const int64_t s = t / nb;
        const int64_t f = (4 * s + (l >> 4)) * vec + e;
        const int c = 16 * b + (l & 15);
        Wp[i] = f < d && c < C1 ? W[(int64_t)c * d + f] : 0.0;
    }
}

// One butterfly step of the (value, index) argmax over a DPP row: the partner's pair wins when its
// value is larger, or equal at a lower index. Both partners end with the same pair.
template <int CTRL>
__device__ __forceinline__ void mm_argmax_step(double& v, int& i) {
    const double pv = dpp_mov<CTRL>(v);
    const int pi = __builtin_amdgcn_mov_dpp(i, CTRL, 0xF, 0xF, true);
    const bool take = pv > v || (pv == v && pi < i);
    v = take ? pv : v;
    i = take ? pi : i;
}

// Tiles [t_lo, t_hi): the multipliers of tile t's row r into mult[((t - t_lo) tile_rows + (r - r0)) C1
// + c] and the tile's {loss, count} into lrec. LDS: the packed W when LDSB.
template <typename S, int NB, bool LDSB>
__global__ __launch_bounds__(kMmBlock) void grad_mn_rowmult_mfma(const ChainDesc* __restrict__ descs,
                                                                 const int64_t* __restrict__ tile0, int P,
                                                                 int64_t t_lo, int64_t t_hi, MnGradGeom gm,
                                                                 const double* __restrict__ Wp,
                                                                 double* __restrict__ mult,
                                                                 double* __restrict__ lrec) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    extern __shared__ double mm_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = gm.d, C1 = gm.C1;
    const int nsteps = gm.dpad / (4 * VEC);
    if constexpr (LDSB) {
        const int total = gm.dpad * 16 * NB;   // a multiple of 128
        for (int i = 2 * (int)threadIdx.x; i < total; i += 2 * kMmBlock) {
            const f64x2 v = *reinterpret_cast<const f64x2*>(Wp + i);
            *reinterpret_cast<f64x2*>(mm_lds + i) = v;
        }
        __syncthreads();
    }
    const int m = lane & 15, q = lane >> 4;
    const int nvec = gm.nvec;                   // the row's vectors that hold a feature (<= ld / VEC)
    const double ninf = -__builtin_inf();
    for (int64_t tile = t_lo + (int64_t)blockIdx.x * kMmWaves + wave; tile < t_hi;
         tile += (int64_t)gridDim.x * kMmWaves) {
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        double* mt = mult + (tile - t_lo) * gm.tile_rows * C1;
        double loss_acc = 0.0;   // (the same in every lane)
        for (int64_t rb = r0; rb < r1; rb += 16) {
            const int64_t row = rb + m;
            const int64_t rr = row < r1 ? row : dsc.n_rows - 1;
            const int64_t ri = dsc.rows ? (int64_t)dsc.rows[rr] : rr;
            const gptr<V> xr =
                as_global(reinterpret_cast<const V*>(reinterpret_cast<const S*>(dsc.x) + ri * dsc.ld));
            mm_d4 acc[NB];
#pragma unroll
            for (int c = 0; c < NB; ++c) acc[c] = mm_d4{0.0, 0.0, 0.0, 0.0};

            // A stage's loads carry no branch: a vector past the row's last loads the last (in bounds at
            // the row's own pitch), and what it holds at a feature >= d is replaced at its use.
            auto load = [&](V (&xv)[kMmU], int s0) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < kMmU; ++u) {
                    const int vi = 4 * (s0 + u) + q;
                    xv[u] = xr[vi < nvec ? vi : nvec - 1];
                }
            };
            auto compute = [&](const V (&xv)[kMmU], int s0) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < kMmU; ++u) {
                    const int s = s0 + u;
                    if (s >= nsteps) break;   // (uniform)
                    double a[VEC];
                    unpack<S, double>(xv[u], a);
                    const int f0 = (4 * s + q) * VEC;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) a[e] = f0 + e < d ? a[e] : 0.0;
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
#pragma unroll
                        for (int c = 0; c < NB; ++c) {
                            double b;
                            if constexpr (LDSB)
                                b = mm_lds[((s * NB + c) * VEC + e) * 64 + lane];
                            else
                                b = as_global(Wp)[(((int64_t)s * NB + c) * VEC + e) * 64 + lane];
                            acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], b, acc[c], 0, 0, 0);
                        }
                }
            };
            // two sets of vectors: the next stage's loads are in flight under this stage's MFMAs
            V xa[kMmU], xb[kMmU];
            int s0 = 0;
            load(xa, 0);
            while (s0 < nsteps) {
                load(xb, s0 + kMmU);
                compute(xa, s0);
                s0 += kMmU;
                if (s0 >= nsteps) break;
                load(xa, s0 + kMmU);
                compute(xb, s0);
                s0 += kMmU;
            }

            // D[q + 4 g][16 c + m]: the lane's class of each block against rows q, q + 4, q + 8, q + 12
            double rl[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t r = rb + q + 4 * g;
                const bool live = r < r1;
                const double yy = as_global(dsc.y)[live ? r : r1 - 1];
                const int ly = mn_d2i(yy) - 1;
                // the maximum: the lane's blocks in ascending order, then the 16 lanes of the DPP row
                double M = ninf;
                int maxIdx = m;
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const int cls = 16 * c + m;
                    const double v = cls < C1 ? acc[c][g] : ninf;
                    const bool take = v > M;
                    M = take ? v : M;
                    maxIdx = take ? cls : maxIdx;
                }
                mm_argmax_step<0xB1>(M, maxIdx);    // quad_perm [1,0,3,2]
                mm_argmax_step<0x4E>(M, maxIdx);    // quad_perm [2,3,0,1]
                mm_argmax_step<0x141>(M, maxIdx);   // row_half_mirror
                mm_argmax_step<0x140>(M, maxIdx);   // row_mirror
                const bool shift = M > 0.0;
                const double eM = exp(-M);
                double ex[NB];
                double part = 0.0, my = 0.0;
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const int cls = 16 * c + m;
                    const double a = acc[c][g];
                    ex[c] = exp(shift ? a - M : a);
                    const double term = shift && cls == maxIdx ? eM : ex[c];
                    part = part + (cls < C1 ? term : 0.0);
                    my = cls < C1 && cls == ly ? a : my;
                }
                // over the DPP row, every lane the same bits; one lane at most holds the label's margin
                const double sum = group_sum(part, 16);
                const double marginY = group_sum(my, 16);
                rl[g] = live ? mn_loss(sum, marginY, M, yy) : 0.0;
                const double den = sum + 1.0;
                double* mr = mt + (rb - r0 + q + 4 * g) * C1;   // (< tile_rows: a multiple of 16)
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const int cls = 16 * c + m;
                    if (cls < C1) mr[cls] = live ? ex[c] / den - mn_indicator(yy, cls) : 0.0;
                }
            }
            // the group's losses in row order: row r sits in DPP row r & 3, register r >> 2
#pragma unroll
            for (int r = 0; r < 16; ++r) loss_acc += readlane_d(rl[r >> 2], 16 * (r & 3));
        }
        if (lane == 0) {
            lrec[2 * tile] = loss_acc;
            lrec[2 * tile + 1] = r1 > r0 ? (double)(r1 - r0) : 0.0;
        }
    }
}

// Tiles [t_lo, t_hi) cut into pieces of `piece` = min(span, range) tiles (powers of two, t_lo a
// multiple of range: a piece lies inside one span). Item (piece, rectangle C of the features): the
// wave adds mult^T x over the piece's rows in order -- from zero at a span's first piece, else from the
// span's record -- and leaves the span's record rec[span][C1 d].
template <typename S, int GR, int GC>
__global__ __launch_bounds__(kMmSumBlock, 1) void grad_mn_wsum_mfma(const ChainDesc* __restrict__ descs,
                                                                   const int64_t* __restrict__ tile0, int P,
                                                                   int64_t t_lo, int64_t t_hi, int64_t piece,
                                                                   int64_t n_items, MnGradGeom gm,
                                                                   const double* __restrict__ mult, double* rec) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t item = (int64_t)blockIdx.x * kMmSumWaves + wave;
    if (item >= n_items) return;
    const int64_t pc = item / gm.ncg;
    const int kb0 = (int)(item - pc * gm.ncg) * GC;
    const int64_t tb = t_lo + pc * piece;
    const int64_t te = tb + piece < t_hi ? tb + piece : t_hi;
    const int d = gm.d, C1 = gm.C1;
    const int nbf = (d + 15) / 16;
    // block (r, c) of the rectangle is computed when it lies inside [classes] x [features]
    unsigned on = 0;
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c)
            if (r < gm.nb && kb0 + c < nbf) on |= 1u << (r * GC + c);
    on = __builtin_amdgcn_readfirstlane(on);
    const int m = lane & 15, kq = lane >> 4;
    // the lane's class of each A fragment (one >= C1 loads class 0; its value is not used); its column
    // of each B fragment and the feature it loads (a column >= d loads feature d - 1, in bounds and
    // never a pad column; its value is not used)
    int cen[GR], cl[GR], cb[GC], lb[GC];
#pragma unroll
    for (int r = 0; r < GR; ++r) {
        cen[r] = r * 16 + m;
        cl[r] = cen[r] < C1 ? cen[r] : 0;
    }
#pragma unroll
    for (int c = 0; c < GC; ++c) {
        cb[c] = (kb0 + c) * 16 + m;
        lb[c] = cb[c] < d ? cb[c] : d - 1;
    }
    // D[class 16 r + kq + 4 g][feature cb[c]] is the lane's register g of block (r, c)
    double* out = rec + (tb / gm.span) * ((int64_t)C1 * d);
    const bool first = tb % gm.span == 0;
    mm_d4 acc[GR][GC];
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int cls = r * 16 + kq + 4 * g;
                const bool cell = cls < C1 && cb[c] < d;
                acc[r][c][g] = !first && cell ? out[(int64_t)cls * d + cb[c]] : 0.0;
            }

    for (int64_t tile = tb; tile < te; ++tile) {
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        if (r1 <= r0) continue;   // (a sampled batch's tiles past its end)
        const S* X = reinterpret_cast<const S*>(dsc.x);
        const double* mt = mult + (tile - t_lo) * gm.tile_rows * C1;
        // A stage's loads carry no lane-conditional branch and no conversion: a row past the tile's end
        // loads its last row, and the selection at the use keeps it out of the sums.
        auto load = [&](S (&fb)[kMmSub][GC], double (&fa)[kMmSub][GR], int64_t rb) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < kMmSub; ++s) {
                const int64_t row = rb + 4 * s + kq;
                const int64_t rr = row < r1 ? row : r1 - 1;
                const int64_t ri = dsc.rows ? (int64_t)dsc.rows[rr] : rr;
                const gptr<S> xr = as_global(X + ri * dsc.ld);
#pragma unroll
                for (int c = 0; c < GC; ++c) fb[s][c] = xr[lb[c]];
                const gptr<double> mr = as_global(mt + (rr - r0) * C1);
#pragma unroll
                for (int r = 0; r < GR; ++r) fa[s][r] = mr[cl[r]];
            }
        };
        auto compute = [&](const S (&fb)[kMmSub][GC], const double (&fa)[kMmSub][GR], int64_t rb)
                           __attribute__((always_inline)) {
            unsigned onl = __builtin_amdgcn_readfirstlane(on);
            asm volatile("" : "+s"(onl));
#pragma unroll
            for (int s = 0; s < kMmSub; ++s) {
                const bool valid = rb + 4 * s + kq < r1;
                double a[GR], b[GC];
#pragma unroll
                for (int r = 0; r < GR; ++r) a[r] = valid && cen[r] < C1 ? fa[s][r] : 0.0;
#pragma unroll
                for (int c = 0; c < GC; ++c) b[c] = cb[c] < d ? (double)fb[s][c] : 0.0;
#pragma unroll
                for (int r = 0; r < GR; ++r)
#pragma unroll
                    for (int c = 0; c < GC; ++c)
                        if ((onl >> (r * GC + c)) & 1u)
                            acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[c], acc[r][c], 0, 0, 0);
            }
        };
        // two sets of fragments: the next stage's loads are in flight under this stage's MFMAs
        constexpr int64_t stage = 4 * kMmSub;
        S xa[kMmSub][GC], xb[kMmSub][GC];
        double ma[kMmSub][GR], mb[kMmSub][GR];
        int64_t rb = r0;
        load(xa, ma, rb);
        while (rb < r1) {
            load(xb, mb, rb + stage);
            compute(xa, ma, rb);
            rb += stage;
            if (rb >= r1) break;
            load(xa, ma, rb + stage);
            compute(xb, mb, rb);
            rb += stage;
        }
    }
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c)
            if ((on >> (r * GC + c)) & 1u) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int cls = r * 16 + kq + 4 * g;
                    if (cls < C1 && cb[c] < d) out[(int64_t)cls * d + cb[c]] = acc[r][c][g];
                }
            }
}

template <typename K, typename... A>
int mm_launch(K kern, unsigned blocks, int threads, int64_t lds, hipStream_t st, A... args) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), (size_t)lds, st, args...);
    return (int)hipGetLastError();
}

template <typename S, bool LDSB, typename... A>
int rowmult_nb(int nb, unsigned blocks, int64_t lds, hipStream_t st, A... args) {
    switch (nb) {
        case 1: return mm_launch(grad_mn_rowmult_mfma<S, 1, LDSB>, blocks, kMmBlock, lds, st, args...);
        case 2: return mm_launch(grad_mn_rowmult_mfma<S, 2, LDSB>, blocks, kMmBlock, lds, st, args...);
        case 3: return mm_launch(grad_mn_rowmult_mfma<S, 3, LDSB>, blocks, kMmBlock, lds, st, args...);
        case 4: return mm_launch(grad_mn_rowmult_mfma<S, 4, LDSB>, blocks, kMmBlock, lds, st, args...);
    }
    return (int)hipErrorInvalidValue;
}

template <typename S, typename... A>
int wsum_rect(const MnGradGeom& gm, unsigned blocks, hipStream_t st, A... args) {
    switch (gm.gr * 16 + gm.gc) {
        case 1 * 16 + 2: return mm_launch(grad_mn_wsum_mfma<S, 1, 2>, blocks, kMmSumBlock, 0, st, args...);
        case 1 * 16 + 8: return mm_launch(grad_mn_wsum_mfma<S, 1, 8>, blocks, kMmSumBlock, 0, st, args...);
        case 2 * 16 + 2: return mm_launch(grad_mn_wsum_mfma<S, 2, 2>, blocks, kMmSumBlock, 0, st, args...);
        case 2 * 16 + 8: return mm_launch(grad_mn_wsum_mfma<S, 2, 8>, blocks, kMmSumBlock, 0, st, args...);
        case 4 * 16 + 2: return mm_launch(grad_mn_wsum_mfma<S, 4, 2>, blocks, kMmSumBlock, 0, st, args...);
        case 4 * 16 + 8: return mm_launch(grad_mn_wsum_mfma<S, 4, 8>, blocks, kMmSumBlock, 0, st, args...);
    }
    return (int)hipErrorInvalidValue;
}

template <typename S>
int launch_passes_s(const MnGradGeom& gm, int num_cus, hipStream_t st, const ChainDesc* descs, const int64_t* tile0,
                    int P, int64_t n_tiles, const double* wp, double* rec, double* lrec, double* mult) {
    const int64_t lds = gm.wlds ? (int64_t)grad_mn_mfma_pack_doubles(gm) * (int64_t)sizeof(double) : 0;
    // whole workgroups a CU: as many as its LDS holds, four of eight waves at most; whole rounds of them
    const int64_t per_cu = lds > 0 ? std::max<int64_t>(1, std::min<int64_t>(4, kMmLds / lds)) : 4;
    const int64_t cap = per_cu * (num_cus > 0 ? num_cus : 256) * kMmWaves;
    const int64_t piece = std::min<int64_t>(gm.span, gm.range);
    for (int64_t t_lo = 0; t_lo < n_tiles; t_lo += gm.range) {
        const int64_t t_hi = std::min<int64_t>(t_lo + gm.range, n_tiles);
        const int64_t n = t_hi - t_lo;
        const int64_t rounds = (n + cap - 1) / cap;
        const int64_t waves = (n + rounds - 1) / rounds;
        const unsigned blocks = (unsigned)((waves + kMmWaves - 1) / kMmWaves);
        int e = gm.wlds ? rowmult_nb<S, true>(gm.nb, blocks, lds, st, descs, tile0, P, t_lo, t_hi, gm, wp, mult, lrec)
                        : rowmult_nb<S, false>(gm.nb, blocks, 0, st, descs, tile0, P, t_lo, t_hi, gm, wp, mult, lrec);
        if (e) return e;
        const int64_t n_items = (n + piece - 1) / piece * gm.ncg;
        e = wsum_rect<S>(gm, (unsigned)((n_items + kMmSumWaves - 1) / kMmSumWaves), st, descs, tile0, P, t_lo, t_hi,
                         piece, n_items, gm, (const double*)mult, rec);
        if (e) return e;
    }
    return 0;
}

}  // namespace

void grad_mn_mfma_geometry(MnGradGeom& gm, int storage) {
    const int fchunk = 4 * (storage == 1 ? 4 : 2);
    gm.dpad = (gm.d + fchunk - 1) / fchunk * fchunk;
    gm.nb = (gm.C1 + 15) / 16;
    gm.group = 16;
    gm.wlds = (int64_t)grad_mn_mfma_pack_doubles(gm) * (int64_t)sizeof(double) <= kMmLds ? 1 : 0;
    // the smallest built rectangle that holds the class blocks, 4 x 8 (256 accumulator registers) at most
    const int nbf = (gm.d + 15) / 16;
    gm.gr = gm.nb == 1 ? 1 : gm.nb == 2 ? 2 : 4;
    gm.gc = nbf <= 2 ? 2 : 8;
    gm.ncg = (nbf + gm.gc - 1) / gm.gc;
    gm.n_colchunks = gm.ncg;
    gm.n_classchunks = 1;
    // a record of 16 gr d doubles over gr tiles: at most 3.2 % of the tiles' rows
    gm.span = gm.gr;
}

size_t grad_mn_mfma_pack_doubles(const MnGradGeom& gm) { return (size_t)gm.dpad * 16 * (size_t)gm.nb; }

int launch_gradient_mn_mfma(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                            const MnGradGeom& gm, int storage, const double* w, double* rec, double* lrec,
                            double* mult, double* wp, int num_cus, hipStream_t st) {
    const int64_t total = (int64_t)grad_mn_mfma_pack_doubles(gm);
    const unsigned pb = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(grad_mn_pack_w, dim3(pb), dim3(256), 0, st, w, gm.d, gm.C1, gm.nb, storage == 1 ? 4 : 2, total, wp);
    const int e = (int)hipGetLastError();
    if (e) return e;
    return storage == 1 ? launch_passes_s<float>(gm, num_cus, st, descs, tile0, n_parts, n_tiles, wp, rec, lrec, mult)
                        : launch_passes_s<double>(gm, num_cus, st, descs, tile0, n_parts, n_tiles, wp, rec, lrec, mult);
}

}  // namespace psgd
