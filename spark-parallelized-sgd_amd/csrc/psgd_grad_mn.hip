// psgd_grad_mn.hip -- the batch gradient of the multinomial LogisticGradient (numClasses = K > 2) at
// fixed weights over the registered partitions (psgd_gradient_sum_multinomial): what MLlib 1.6.1's
// GradientDescent.runMiniBatchSGD sums per iteration for a multiclass model, in fp64 whatever the
// storage. With C1 = K - 1 class blocks W[c d + j] (class 0 the pivot) a row (x, y) has margins
// m_c = sum_j x_j W[c d + j], the maximum M (first index on ties; a positive M shifts every margin
// and puts exp(-M) in its own place in the sum), multipliers mult_c = exp(m_c [- M]) / (sum + 1) -
// [y != 0 and y == c + 1] and the loss of psgd_eval_mn.hip (oracle/psgd_ref.py::multinomial).
// out = {gradientSum[c d + j] = sum_i mult_ic x_ij, lossSum, count}: C1 d + 2 doubles.
//
// The tiling, the sampled-batch convention (ChainDesc::rows: tile t holds samples [t tile_rows,
// (t + 1) tile_rows) of the batch, tiles past the batch's end are empty) and the {loss, count}
// record a tile are psgd_grad.hip's; grad_merge adds the records in tile order.
//
// Dense rows: no floating-point atomics, the same bits from call to call; the sum order is fixed by
// the registry's geometry and K.
//   Fused (grad_mn_fused): where C1 <= 16 and a lane's cp x nvl accumulator vectors (cp = C1 rounded
//   up to 2, 4, 8, 16; nvl = 16-byte row vectors a lane owns) number at most kGmFusedVecs = 16, i.e.
//   at most 64 fp64 accumulators -- and, of those shapes, where it was measured faster than the
//   general path (grad_mn_geometry has the rule). A work item is a tile; lanes lie across a row's vectors as in
//   grad_dense. A row is read from HBM once: a wave widens up to 64 rows into registers, takes their
//   margins against the class blocks in LDS (f64, always within budget: C1 x pitch <= 4,096
//   doubles; a weight read serves the group's rows), parks them, lane i turns row i's margins into
//   its multipliers (once a row), and every lane adds mult_c . x into its accumulators from the
//   registers that still hold the rows. A tile ends with a record of C1 d doubles.
//   General (every other dense shape, and PSGD_GRAD_MN_TWO_PASS=1): the batch is taken in ranges of
//   `range` tiles. grad_mn_rowmult writes mult[rows of the range, C1] and every tile's {loss, count}
//   (score_dense_mn's register hold and class loop; the class blocks in LDS while C1 x pitch <=
//   kMnWLds; one lane a row's softmax while C1 <= kMnLaneClasses, else the lanes across the classes).
//   grad_mn_wsum then runs over (tile span, column chunk, class chunk) items: a lane owns 2 row
//   vectors x 8 classes of accumulators and walks the rows of its span in order; narrow rows put
//   64 / agroup class chunks side by side in a wave. A span is `span` = the power of two >= C1 / 16
//   consecutive tiles, one record each; when a range is shorter than a span the item continues from
//   the span's record, so the order of the sum does not depend on the range.
//   Scratch, in doubles, T tiles, n = ceil(T / span) gradient records (span = 1 when fused):
//       (n + ceil(n / 32) + 1) C1 d  +  (T + ceil(T / 32) + 1) 2  +  min(range, T) tile_rows C1
//   with C1 / span <= 16 (records: at most 3.2 % of the rows' bytes beside one record) and
//   range tile_rows C1 <= max(kGmMultDoubles = 2^25, tile_rows C1) (multipliers: 256 MiB, or one tile's).
//   Neither span nor range changes a bit of the result's order within a span; PSGD_GRAD_MN_RANGE=n
//   (tests) shortens the ranges to at most n tiles.
//
// CSR rows, gradientSum NOT bitwise reproducible (lossSum and count are): one pass as grad_csr. A
// wave gathers the margins of the rows its buffer holds in score_csr_mn's entry loop, turns them into
// multipliers, and visits the rows again (from cache) adding mult_c . val into out[c d + col] with
// fp64 vector atomics -- in an LDS accumulator flushed once a workgroup when C1 d <= kGradLdsFeatures
// (grad_csr_lds_applies: PSGD_GRAD_CSR_GLOBAL=1 forces the global path).
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include <algorithm>
#include <cstdlib>

#include "psgd_device.h"
#include "psgd_eval.h"

namespace psgd {
namespace {

constexpr int kGmBlock = 256;
constexpr int kGmWaves = kGmBlock / 64;
constexpr int kGmFusedVecs = 16;           // fused: cp x nvl at most (64 f32-row / 32 f64-row accumulators a lane)
constexpr int kGmFusedClasses = 16;        // fused: C1 at most
constexpr int kGmChunkVecs = 2;            // accumulation pass: row vectors a lane owns
constexpr int kGmChunkClasses = 8;         // accumulation pass: classes a lane owns
constexpr int64_t kGmMultDoubles = 1ll << 25;   // multipliers a range holds (256 MiB)
constexpr int kGmCsrWaves = 8;

__device__ __forceinline__ double mn_indicator(double y, int c) {
    return (y != 0.0 && y == (double)(c + 1)) ? 1.0 : 0.0;
}

// Row-per-lane: rows row0 .. row0 + n (n <= 64) of the batch at marg[i * pitch + c]; lane i replaces
// row i's margins by its multipliers, classes in order (the reference's order), and adds its loss.
// Rows at or past r1 get multipliers 0.
__device__ __forceinline__ void mn_mult_rows(double* marg, int n, int pitch, int C1, const double* __restrict__ y,
                                             int64_t row0, int64_t r1, int lane, double& loss_acc) {
    wave_lds_sync();
    if (lane < n) {
        double* m = marg + lane * pitch;
        if (row0 + lane < r1) {
            const double yy = y[row0 + lane];
            const int ly = mn_d2i(yy) - 1;
            double marginY = 0.0, M = -__builtin_inf();
            int maxIdx = 0;
            for (int c = 0; c < C1; ++c) {
                const double v = m[c];
                if (c == ly) marginY = v;
                if (v > M) {
                    M = v;
                    maxIdx = c;
                }
            }
            const bool shift = M > 0.0;
            double sum = 0.0;
            for (int c = 0; c < C1; ++c) {
                if (shift) sum = sum + (c == maxIdx ? exp(-M) : exp(m[c] - M));
                else sum = sum + exp(m[c]);
            }
            loss_acc += mn_loss(sum, marginY, M, yy);
            const double den = sum + 1.0;
            for (int c = 0; c < C1; ++c) {
                const double e = shift ? exp(m[c] - M) : exp(m[c]);
                m[c] = e / den - mn_indicator(yy, c);
            }
        } else {
            for (int c = 0; c < C1; ++c) m[c] = 0.0;
        }
    }
    wave_lds_sync();
}

// Lanes across the classes: rows row0 .. row0 + n at marg[i * C1 + c], a row at a time (every one
// of them before r1).
__device__ __forceinline__ void mn_mult_wide(double* marg, int n, int C1, const double* __restrict__ y, int64_t row0,
                                             int lane, double& loss_acc) {
    wave_lds_sync();
    for (int i = 0; i < n; ++i) {
        double* m = marg + (int64_t)i * C1;
        const double yy = y[row0 + i];
        const int ly = mn_d2i(yy) - 1;
        double M = -__builtin_inf();
        int maxIdx = 0x7fffffff;
        for (int c = lane; c < C1; c += 64) {
            const double v = m[c];
            if (v > M) {
                M = v;
                maxIdx = c;
            }
        }
        // the maximum, the lowest class among equals
        for (int s = 1; s < 64; s <<= 1) {
            const double vo = __shfl_xor(M, s, 64);
            const int io = __shfl_xor(maxIdx, s, 64);
            if (vo > M || (vo == M && io < maxIdx)) {
                M = vo;
                maxIdx = io;
            }
        }
        if (maxIdx == 0x7fffffff) maxIdx = 0;   // (no margin compares: NaNs)
        const bool shift = M > 0.0;
        double part = 0.0;
        for (int c = lane; c < C1; c += 64) {
            if (shift) part = part + (c == maxIdx ? exp(-M) : exp(m[c] - M));
            else part = part + exp(m[c]);
        }
        const double sum = wave_sum(part);
        const double marginY = (ly >= 0 && ly < C1) ? m[ly] : 0.0;
        if (lane == 0) loss_acc += mn_loss(sum, marginY, M, yy);
        const double den = sum + 1.0;
        wave_lds_sync();   // (marginY is read before the row's margins are replaced)
        for (int c = lane; c < C1; c += 64) {
            const double e = shift ? exp(m[c] - M) : exp(m[c]);
            m[c] = e / den - mn_indicator(yy, c);
        }
    }
    wave_lds_sync();
}

// Rows of a lane group in one set of row registers: 8 vectors a lane at most, widened to f64.
template <int NVL>
constexpr int mn_fused_rows() { return NVL >= 8 ? 1 : NVL >= 4 ? 2 : 4; }

// LDS: [class blocks, C1 x wp doubles, wp = gl NVL VEC (zeros past d) | a margin buffer of 64 rows
// at pitch C1 | 1 per wave].
template <typename S, int NVL, int CP>
__global__ __launch_bounds__(kGmBlock) void grad_mn_fused(const ChainDesc* __restrict__ descs,
                                                          const int64_t* __restrict__ tile0, int P, int64_t n_tiles,
                                                          MnGradGeom gm, const double* __restrict__ w,
                                                          double* __restrict__ rec, double* __restrict__ lrec) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int R = mn_fused_rows<NVL>();
    extern __shared__ __attribute__((aligned(16))) double mn_lds[];
    const int d = gm.d, C1 = gm.C1;
    const int gl = gm.group, rpw = 64 / gl;
    const int wp = gl * NVL * VEC;
    for (int i = threadIdx.x; i < C1 * wp; i += kGmBlock) {
        const int c = i / wp, f = i - c * wp;
        mn_lds[i] = f < d ? w[(int64_t)c * d + f] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = lane / gl, j = lane & (gl - 1);
    const int pitch = C1 | 1;
    double* buf = mn_lds + C1 * wp + wave * 64 * pitch;
    const int ract = R < gl ? R : gl;   // the wave's rows of one round are at most 64 (one a lane)
    const int round = rpw * ract;
    const int nfull = d / VEC, rem = d - nfull * VEC;
    int vc[NVL];
    bool vok[NVL];
#pragma unroll
    for (int u = 0; u < NVL; ++u) {
        const int v = u * gl + j;
        vok[u] = v < gm.nvec;
        vc[u] = vok[u] ? v : 0;   // (a vector past the row's last reads vector 0 instead, times weights of 0.0)
    }
    const int64_t Wg = (int64_t)C1 * d;
    for (int64_t tile = (int64_t)blockIdx.x * kGmWaves + wave; tile < n_tiles;
         tile += (int64_t)gridDim.x * kGmWaves) {
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        double G[CP][NVL][VEC];
#pragma unroll
        for (int c = 0; c < CP; ++c)
#pragma unroll
            for (int u = 0; u < NVL; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) G[c][u][e] = 0.0;
        double loss_acc = 0.0;
        V raw[R][NVL];
        auto load = [&](int64_t rb) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < R; ++q) {
                if (q < ract) {
                    const int64_t r = rb + (int64_t)q * rpw + g;
                    // (a lane group past the tile's end re-reads its first row; its multipliers are 0)
                    const int64_t rr = r < r1 ? r : r0;
                    const int64_t ri = dsc.rows ? (int64_t)dsc.rows[rr] : rr;
                    const V* row = reinterpret_cast<const V*>(X + ri * dsc.ld);
#pragma unroll
                    for (int u = 0; u < NVL; ++u) raw[q][u] = __builtin_nontemporal_load(as_global(row + vc[u]));
                }
            }
        };
        if (r0 < r1) load(r0);
        for (int64_t rb = r0; rb < r1; rb += round) {
            double x[R][NVL][VEC];
#pragma unroll
            for (int q = 0; q < R; ++q)
#pragma unroll
                for (int u = 0; u < NVL; ++u) {
                    unpack<S, double>(raw[q][u], x[q][u]);
                    // the pad of the row's partial vector is the caller's (zero-copy rows): not used;
                    // a vector past the row's last adds nothing to the accumulators that are written
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
                        if (!vok[u] || (rem && vc[u] == nfull && e >= rem)) x[q][u][e] = 0.0;
                }
            if (rb + round < r1) load(rb + round);   // the next round's rows, under this round's arithmetic
#pragma unroll 1
            for (int c = 0; c < C1; ++c) {
                const double* wc = mn_lds + c * wp + j * VEC;
                double acc[R];
#pragma unroll
                for (int q = 0; q < R; ++q) acc[q] = 0.0;
#pragma unroll
                for (int u = 0; u < NVL; ++u) {
                    double wk[VEC];
                    const f64x2* w2 = reinterpret_cast<const f64x2*>(wc + u * gl * VEC);
#pragma unroll
                    for (int h = 0; h < VEC / 2; ++h) {
                        const f64x2 t = w2[h];
                        wk[2 * h] = t[0];
                        wk[2 * h + 1] = t[1];
                    }
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
#pragma unroll
                        for (int q = 0; q < R; ++q) acc[q] = __builtin_fma(x[q][u][e], wk[e], acc[q]);
                }
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    if (q < ract) {
                        const double dot = group_sum(acc[q], gl);
                        if (j == 0) buf[(q * rpw + g) * pitch + c] = dot;
                    }
                }
            }
            mn_mult_rows(buf, round, pitch, C1, dsc.y, rb, r1, lane, loss_acc);
#pragma unroll
            for (int q = 0; q < R; ++q) {
                if (q < ract) {
                    const double* mq = buf + (q * rpw + g) * pitch;
#pragma unroll
                    for (int c = 0; c < CP; ++c) {
                        if (c < C1) {
                            const double m = mq[c];
#pragma unroll
                            for (int u = 0; u < NVL; ++u)
#pragma unroll
                                for (int e = 0; e < VEC; ++e) G[c][u][e] = __builtin_fma(m, x[q][u][e], G[c][u][e]);
                        }
                    }
                }
            }
            wave_lds_sync();   // the next round's margins overwrite the multipliers
        }
        // narrow rows: the wave's 64 / gl lane groups hold different rows of the same columns
        for (int m = gl; m < 64; m <<= 1) {
#pragma unroll
            for (int c = 0; c < CP; ++c)
#pragma unroll
                for (int u = 0; u < NVL; ++u)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) G[c][u][e] += __shfl_xor(G[c][u][e], m, 64);
        }
        loss_acc = wave_sum(loss_acc);
        double* out = rec + tile * Wg;
        if (g == 0) {
#pragma unroll
            for (int c = 0; c < CP; ++c)
#pragma unroll
                for (int u = 0; u < NVL; ++u)
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const int col = vc[u] * VEC + e;
                        if (c < C1 && vok[u] && col < d) out[(int64_t)c * d + col] = G[c][u][e];
                    }
        }
        if (lane == 0) {
            lrec[2 * tile] = loss_acc;
            lrec[2 * tile + 1] = r1 > r0 ? (double)(r1 - r0) : 0.0;
        }
    }
}

// General path, pass 1 over tiles [t_lo, t_hi): the multipliers of tile t's row r into
// mult[((t - t_lo) tile_rows + (r - r0)) C1 + c] and the tile's {loss, count} into lrec. LDS: [the
// class blocks at pitch dp when WLDS (wpad doubles) | a margin buffer of mb doubles per wave].
template <typename S, bool WLDS, bool ROWLANE>
__global__ __launch_bounds__(kGmCsrWaves * 64) void grad_mn_rowmult(const ChainDesc* __restrict__ descs,
                                                                    const int64_t* __restrict__ tile0, int P,
                                                                    int64_t t_lo, int64_t t_hi, MnGradGeom gm,
                                                                    const double* __restrict__ w, int mb, int wpad,
                                                                    double* __restrict__ mult,
                                                                    double* __restrict__ lrec) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int XH = kMnHold / VEC;   // vectors of a row a lane holds
    constexpr int R = kMnRows;
    extern __shared__ __attribute__((aligned(16))) double mn_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_waves = (int)(blockDim.x >> 6);
    const int d = gm.d, C1 = gm.C1, nvec = gm.nvec;
    const int dp = nvec * VEC;          // a class block's pitch in LDS: whole vectors, zeros past d
    if constexpr (WLDS) {
        for (int i = threadIdx.x; i < C1 * dp; i += blockDim.x) {
            const int c = i / dp, f = i - c * dp;
            mn_lds[i] = f < d ? w[(int64_t)c * d + f] : 0.0;
        }
        __syncthreads();
    }
    double* marg = mn_lds + (WLDS ? wpad : 0) + (int64_t)wave * mb;
    const int gl = gm.group;
    int pitch, rp, nb;
    mn_buffer_shape<ROWLANE>(C1, 64 / gl, R, pitch, rp, nb);
    const int g = lane / gl, j = lane & (gl - 1);
    const int n_chunks = (nvec + gl * XH - 1) / (gl * XH);
    for (int64_t tile = t_lo + (int64_t)blockIdx.x * n_waves + wave; tile < t_hi;
         tile += (int64_t)gridDim.x * n_waves) {
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        double* mt = mult + (tile - t_lo) * gm.tile_rows * C1;
        int64_t buf_row = r0;   // the batch row of the buffer's first row
        double loss_acc = 0.0;
        for (int64_t rb = r0; rb < r1; rb += (int64_t)rp * R) {
            bool valid[R];
            const V* row[R];
            int slot[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int64_t r = rb + (int64_t)u * rp + g;
                valid[u] = g < rp && r < r1;
                const int64_t rr = valid[u] ? r : r0;   // (a group past the tile's end re-reads its first row)
                const int64_t ri = dsc.rows ? (int64_t)dsc.rows[rr] : rr;
                row[u] = reinterpret_cast<const V*>(X + ri * dsc.ld);
                slot[u] = (int)(rr - buf_row) * pitch;
            }
            for (int ch = 0; ch < n_chunks; ++ch) {
                V xv[R][XH];
                int eo[kMnHold];   // the held elements' features (0 for an element outside the row: its x is 0.0)
                bool in[kMnHold];
#pragma unroll
                for (int t = 0; t < XH; ++t) {
                    const int v = (ch * XH + t) * gl + j;
                    const int vv = v < nvec ? v : 0;
#pragma unroll
                    for (int u = 0; u < R; ++u) xv[u][t] = __builtin_nontemporal_load(as_global(row[u] + vv));
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const int f = v * VEC + e;
                        in[t * VEC + e] = v < nvec && f < d;   // (the last vector's tail lies in the row's pad)
                        eo[t * VEC + e] = in[t * VEC + e] ? f : 0;
                    }
                }
                double x[R][kMnHold];
#pragma unroll
                for (int u = 0; u < R; ++u)
#pragma unroll
                    for (int t = 0; t < XH; ++t) {
                        double xe[VEC];
                        unpack<S, double>(xv[u][t], xe);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) x[u][t * VEC + e] = in[t * VEC + e] ? xe[e] : 0.0;
                    }
#pragma unroll 1
                for (int c = 0; c < C1; ++c) {
                    double acc[R];
#pragma unroll
                    for (int u = 0; u < R; ++u) acc[u] = 0.0;
#pragma unroll
                    for (int t = 0; t < XH; ++t) {
                        double wk[VEC];
                        if constexpr (WLDS) {
                            // 16-byte reads: dp and the vector's first feature are even
                            const f64x2* wq = reinterpret_cast<const f64x2*>(mn_lds + c * dp + eo[t * VEC]);
#pragma unroll
                            for (int h = 0; h < VEC / 2; ++h) {
                                const f64x2 w2 = wq[h];
                                wk[2 * h] = w2[0];
                                wk[2 * h + 1] = w2[1];
                            }
                        } else {
#pragma unroll
                            for (int e = 0; e < VEC; ++e) wk[e] = w[(int64_t)c * d + eo[t * VEC + e]];
                        }
#pragma unroll
                        for (int e = 0; e < VEC; ++e)
#pragma unroll
                            for (int u = 0; u < R; ++u) acc[u] = __builtin_fma(x[u][t * VEC + e], wk[e], acc[u]);
                    }
                    static_assert(R == 2, "group_sum2 reduces the two rows of a group together");
                    group_sum2(acc[0], acc[1], gl);
#pragma unroll
                    for (int u = 0; u < R; ++u) {
                        if (valid[u] && j == 0) {
                            double* mp = marg + slot[u] + c;
                            *mp = ch == 0 ? acc[u] : *mp + acc[u];   // (the lane's own earlier store)
                        }
                    }
                }
            }
            const int64_t next = rb + (int64_t)rp * R;
            if (next - buf_row >= nb || next >= r1) {
                const int64_t end = next < r1 ? next : r1;
                const int n = (int)(end - buf_row);
                if constexpr (ROWLANE) mn_mult_rows(marg, n, pitch, C1, dsc.y, buf_row, r1, lane, loss_acc);
                else mn_mult_wide(marg, n, C1, dsc.y, buf_row, lane, loss_acc);
                double* out = mt + (buf_row - r0) * C1;
                for (int q = lane; q < n * C1; q += 64) out[q] = marg[(q / C1) * pitch + q % C1];
                wave_lds_sync();
                buf_row = end;
            }
        }
        loss_acc = wave_sum(loss_acc);
        if (lane == 0) {
            lrec[2 * tile] = loss_acc;
            lrec[2 * tile + 1] = r1 > r0 ? (double)(r1 - r0) : 0.0;
        }
    }
}

// General path, pass 2 over tiles [t_lo, t_hi), cut into pieces of `piece` = min(span, range) tiles
// (powers of two, t_lo a multiple of range: a piece lies inside one span). A work item is (piece,
// column chunk of agroup * 2 vectors, class chunk of (64 / agroup) * 8 classes): lane (g, j) owns
// vectors j, j + agroup of the chunk and 8 classes from (chunk * 64 / agroup + g) * 8 on, and adds
// mult_c . x over the piece's rows in order -- from zero at a span's first piece, else from the
// span's record.
template <typename S>
__global__ __launch_bounds__(kGmBlock) void grad_mn_wsum(const ChainDesc* __restrict__ descs,
                                                         const int64_t* __restrict__ tile0, int P, int64_t t_lo,
                                                         int64_t t_hi, int64_t piece, int64_t n_items, MnGradGeom gm,
                                                         const double* __restrict__ mult, double* rec) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int U = kGmChunkVecs, CC = kGmChunkClasses, RB = 2;
    const int d = gm.d, C1 = gm.C1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gl = gm.agroup, ng = 64 / gl;
    const int g = lane / gl, j = lane & (gl - 1);
    const int64_t Wg = (int64_t)C1 * d;
    for (int64_t item = (int64_t)blockIdx.x * kGmWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kGmWaves) {
        const int kc = (int)(item % gm.n_classchunks);
        const int64_t t = item / gm.n_classchunks;
        const int cc = (int)(t % gm.n_colchunks);
        const int64_t tb = t_lo + (t / gm.n_colchunks) * piece;
        const int64_t te = tb + piece < t_hi ? tb + piece : t_hi;
        double* out = rec + (tb / gm.span) * Wg;
        const bool first = tb % gm.span == 0;
        const int c0 = (kc * ng + g) * CC;
        int v[U], vc[U];
        bool vok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v[u] = (cc * U + u) * gl + j;
            vok[u] = v[u] < gm.nvec;
            vc[u] = vok[u] ? v[u] : 0;
        }
        double G[CC][U][VEC];
#pragma unroll
        for (int k = 0; k < CC; ++k)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int col = v[u] * VEC + e;
                    const bool live = c0 + k < C1 && vok[u] && col < d;
                    G[k][u][e] = (!first && live) ? out[(int64_t)(c0 + k) * d + col] : 0.0;
                }
        for (int64_t tile = tb; tile < te; ++tile) {
            const int p = tile_partition(tile0, P, tile);
            const ChainDesc dsc = descs[p];
            const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
            const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
            const S* X = reinterpret_cast<const S*>(dsc.x);
            const double* mt = mult + (tile - t_lo) * gm.tile_rows * C1;
            for (int64_t rb = r0; rb < r1; rb += RB) {
                V xv[RB][U];
                double m[RB][CC];
#pragma unroll
                for (int q = 0; q < RB; ++q) {
                    const int64_t r = rb + q;
                    const int64_t rr = r < r1 ? r : r0;
                    const int64_t ri = dsc.rows ? (int64_t)dsc.rows[rr] : rr;
                    const V* row = reinterpret_cast<const V*>(X + ri * dsc.ld);
#pragma unroll
                    for (int u = 0; u < U; ++u) xv[q][u] = __builtin_nontemporal_load(as_global(row + vc[u]));
#pragma unroll
                    for (int k = 0; k < CC; ++k)
                        m[q][k] = (r < r1 && c0 + k < C1) ? mt[(rr - r0) * C1 + c0 + k] : 0.0;
                }
#pragma unroll
                for (int q = 0; q < RB; ++q)
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        double x[VEC];
                        unpack<S, double>(xv[q][u], x);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            // (columns at or past d are never written; their values may be anything)
                            const double xe = vc[u] * VEC + e < d ? x[e] : 0.0;
#pragma unroll
                            for (int k = 0; k < CC; ++k) G[k][u][e] = __builtin_fma(m[q][k], xe, G[k][u][e]);
                        }
                    }
            }
        }
#pragma unroll
        for (int k = 0; k < CC; ++k)
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int col = v[u] * VEC + e;
                    if (c0 + k < C1 && vok[u] && col < d) out[(int64_t)(c0 + k) * d + col] = G[k][u][e];
                }
    }
}

// ---- CSR ----
__device__ __forceinline__ void lds_add(double* p, double v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// LDS: [the workgroup's accumulator of C1 d doubles when LDSACC (apad doubles) | a margin buffer of
// mb doubles per wave].
template <typename S, bool LDSACC, bool ROWLANE>
__global__ __launch_bounds__(kGmCsrWaves * 64) void grad_mn_csr(const ChainDesc* __restrict__ descs,
                                                                const int64_t* __restrict__ tile0, int P,
                                                                int64_t n_tiles, MnGradGeom gm,
                                                                const double* __restrict__ w, int mb, int apad,
                                                                double* out, double* __restrict__ lrec) {
    constexpr int H = kMnCsrHold;
    extern __shared__ __attribute__((aligned(16))) double mn_lds[];
    const int d = gm.d, C1 = gm.C1;
    const int Wg = LDSACC ? C1 * d : 0;
    if constexpr (LDSACC) {
        for (int i = threadIdx.x; i < Wg; i += blockDim.x) mn_lds[i] = 0.0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_waves = (int)(blockDim.x >> 6);
    double* marg = mn_lds + apad + (int64_t)wave * mb;
    const int gl = gm.group, ng = 64 / gl;
    int pitch, rp, nb;
    mn_buffer_shape<ROWLANE>(C1, ng, 1, pitch, rp, nb);
    const int g = lane / gl, j = lane & (gl - 1);
    auto add = [&](int c, int col, double t) __attribute__((always_inline)) {
        if (t != 0.0) {
            if constexpr (LDSACC) lds_add(mn_lds + c * d + col, t);
            else unsafeAtomicAdd(out + (int64_t)c * d + col, t);
        }
    };
    for (int64_t tile = (int64_t)blockIdx.x * n_waves + wave; tile < n_tiles;
         tile += (int64_t)gridDim.x * n_waves) {
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        const S* val = reinterpret_cast<const S*>(dsc.x);
        int64_t buf_row = r0;
        double loss_acc = 0.0;
        for (int64_t rb = r0; rb < r1; rb += rp) {
            const int64_t r = rb + g;
            const bool valid = g < rp && r < r1;
            const int64_t rr = valid ? r : r0;
            const int64_t ri = dsc.rows ? (int64_t)dsc.rows[rr] : rr;
            const int64_t s = dsc.row_ptr[ri];
            const int64_t e = valid ? dsc.row_ptr[ri + 1] : s;
            const int slot = (int)(rr - buf_row) * pitch;
            // every group of the wave loops over the chunks of the wave's longest row
            int64_t len = e - s;
            for (int m = 32; m >= 1; m >>= 1) {
                const int64_t o = __shfl_xor(len, m, 64);
                len = o > len ? o : len;
            }
            const int n_chunks = len > 0 ? (int)((len + (int64_t)gl * H - 1) / ((int64_t)gl * H)) : 1;
            for (int ch = 0; ch < n_chunks; ++ch) {
                double x[H];
                int col[H];
#pragma unroll
                for (int t = 0; t < H; ++t) {
                    const int64_t k = s + ((int64_t)ch * H + t) * gl + j;
                    const bool in = k < e;
                    x[t] = in ? (double)val[k] : 0.0;
                    col[t] = in ? dsc.col[k] : 0;
                }
                for (int c = 0; c < C1; ++c) {
                    const double* wc = w + (int64_t)c * d;
                    double acc = 0.0;
#pragma unroll
                    for (int t = 0; t < H; ++t) acc = __builtin_fma(x[t], wc[col[t]], acc);
                    const double dot = group_sum(acc, gl);
                    if (valid && j == 0) {
                        double* mp = marg + slot + c;
                        *mp = ch == 0 ? dot : *mp + dot;   // (the lane's own earlier store)
                    }
                }
            }
            const int64_t next = rb + rp;
            if (next - buf_row >= nb || next >= r1) {
                const int64_t end = next < r1 ? next : r1;
                const int n = (int)(end - buf_row);
                if constexpr (ROWLANE) mn_mult_rows(marg, n, pitch, C1, dsc.y, buf_row, r1, lane, loss_acc);
                else mn_mult_wide(marg, n, C1, dsc.y, buf_row, lane, loss_acc);
                // the buffer's rows again (from cache): mult_c . val into the accumulator
                if constexpr (ROWLANE) {
                    for (int q = g; q < n; q += ng) {
                        const int64_t qi = dsc.rows ? (int64_t)dsc.rows[buf_row + q] : buf_row + q;
                        const int64_t qe = dsc.row_ptr[qi + 1];
                        const double* mq = marg + q * pitch;
                        for (int64_t k = dsc.row_ptr[qi] + j; k < qe; k += gl) {
                            const double xv = (double)val[k];
                            const int cl = dsc.col[k];
                            for (int c = 0; c < C1; ++c) add(c, cl, mq[c] * xv);
                        }
                    }
                } else {
                    // a row at a time, the lanes across the classes
                    for (int q = 0; q < n; ++q) {
                        const int64_t qi = dsc.rows ? (int64_t)dsc.rows[buf_row + q] : buf_row + q;
                        const int64_t qe = dsc.row_ptr[qi + 1];
                        const double* mq = marg + (int64_t)q * pitch;
                        for (int64_t k = dsc.row_ptr[qi]; k < qe; ++k) {
                            const double xv = (double)val[k];
                            const int cl = dsc.col[k];
                            for (int c = lane; c < C1; c += 64) add(c, cl, mq[c] * xv);
                        }
                    }
                }
                wave_lds_sync();   // the next rows' margins overwrite the multipliers
                buf_row = end;
            }
        }
        loss_acc = wave_sum(loss_acc);
        if (lane == 0) {
            lrec[2 * tile] = loss_acc;
            lrec[2 * tile + 1] = r1 > r0 ? (double)(r1 - r0) : 0.0;
        }
    }
    if constexpr (LDSACC) {
        __syncthreads();
        // 64 consecutive doubles a wave instruction: 512 contiguous bytes of atomics
        for (int i = threadIdx.x; i < Wg; i += blockDim.x) {
            const double v = mn_lds[i];
            if (v != 0.0) unsafeAtomicAdd(out + i, v);
        }
    }
}

template <typename S> constexpr int storage_of() { return sizeof(S) == 4 ? 1 : 0; }

template <typename K, typename... A>
int launch_lds(K k, unsigned blocks, int threads, size_t lds, hipStream_t st, A... args) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k, dim3(blocks), dim3(threads), lds, st, args...);
    return (int)hipGetLastError();
}

template <typename S>
int launch_fused_s(const MnGradGeom& gm, int num_cus, hipStream_t st, const ChainDesc* descs, const int64_t* tile0,
                   int P, int64_t n_tiles, const double* w, double* rec, double* lrec) {
    constexpr int VEC = Vec16<S>::N;
    const size_t lds = ((size_t)gm.C1 * gm.group * gm.nvl * VEC + (size_t)kGmWaves * 64 * (gm.C1 | 1)) * sizeof(double);
    const unsigned blocks = grad_balanced_blocks(n_tiles, num_cus, 2);
#define PSGD_GM_FUSED(NVL, CP)                                                                                    \
    if (gm.nvl == NVL && gm.cp == CP)                                                                             \
        return launch_lds(grad_mn_fused<S, NVL, CP>, blocks, kGmBlock, lds, st, descs, tile0, P, n_tiles, gm, w, \
                          rec, lrec);
    PSGD_GM_FUSED(1, 2) PSGD_GM_FUSED(1, 4) PSGD_GM_FUSED(1, 8) PSGD_GM_FUSED(1, 16)
    PSGD_GM_FUSED(2, 2) PSGD_GM_FUSED(2, 4) PSGD_GM_FUSED(2, 8)
    PSGD_GM_FUSED(4, 2) PSGD_GM_FUSED(4, 4)
    PSGD_GM_FUSED(8, 2)
#undef PSGD_GM_FUSED
    return (int)hipErrorInvalidValue;
}

// The margin buffer of a wave and the waves of a workgroup that fit beside `fixed` doubles of LDS.
void mn_wave_buffers(const MnGradGeom& gm, int rows, int64_t fixed, int* mb, int* waves) {
    *mb = gm.wide ? ((rows * gm.C1 + 1) & ~1) : kMnBuf;
    *waves = kGmCsrWaves;
    if (gm.wide) {
        const int64_t fit = ((int64_t)kMnLdsMax - fixed * 8) / ((int64_t)*mb * 8);
        *waves = (int)(fit < 1 ? 1 : fit > kGmCsrWaves ? kGmCsrWaves : fit);
    }
}

unsigned persistent_blocks(int64_t n_items, int waves, int num_cus) {
    const int64_t want = (n_items + waves - 1) / waves;
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 2 * (kGmCsrWaves / waves);
    return (unsigned)(want < cap ? want : cap);
}

template <typename S>
int launch_general_s(const MnGradGeom& gm, int num_cus, hipStream_t st, const ChainDesc* descs, const int64_t* tile0,
                     int P, int64_t n_tiles, const double* w, double* rec, double* lrec, double* mult) {
    const int wpad = gm.wlds ? (int)(gm.C1 * mn_lds_pitch(gm.d, storage_of<S>())) : 0;   // (even: the pitch is)
    int mb, waves;
    mn_wave_buffers(gm, kMnRows, wpad, &mb, &waves);
    const size_t lds = ((size_t)wpad + (size_t)waves * mb) * sizeof(double);
    const int64_t piece = std::min<int64_t>(gm.span, gm.range);
    for (int64_t t_lo = 0; t_lo < n_tiles; t_lo += gm.range) {
        const int64_t t_hi = std::min<int64_t>(t_lo + gm.range, n_tiles);
        const unsigned blocks = persistent_blocks(t_hi - t_lo, waves, num_cus);
        int e;
        if (gm.wlds && !gm.wide)
            e = launch_lds(grad_mn_rowmult<S, true, true>, blocks, waves * 64, lds, st, descs, tile0, P, t_lo, t_hi, gm, w, mb, wpad, mult, lrec);
        else if (gm.wlds)
            e = launch_lds(grad_mn_rowmult<S, true, false>, blocks, waves * 64, lds, st, descs, tile0, P, t_lo, t_hi, gm, w, mb, wpad, mult, lrec);
        else if (!gm.wide)
            e = launch_lds(grad_mn_rowmult<S, false, true>, blocks, waves * 64, lds, st, descs, tile0, P, t_lo, t_hi, gm, w, mb, wpad, mult, lrec);
        else
            e = launch_lds(grad_mn_rowmult<S, false, false>, blocks, waves * 64, lds, st, descs, tile0, P, t_lo, t_hi, gm, w, mb, wpad, mult, lrec);
        if (e) return e;
        const int64_t n_pieces = (t_hi - t_lo + piece - 1) / piece;
        const int64_t n_items = n_pieces * gm.n_colchunks * gm.n_classchunks;
        hipLaunchKernelGGL(grad_mn_wsum<S>, dim3(grad_balanced_blocks(n_items, num_cus, 4)), dim3(kGmBlock), 0, st, descs,
                           tile0, P, t_lo, t_hi, piece, n_items, gm, mult, rec);
        e = (int)hipGetLastError();
        if (e) return e;
    }
    return 0;
}

template <typename S>
int launch_csr_s(const MnGradGeom& gm, int num_cus, hipStream_t st, const ChainDesc* descs, const int64_t* tile0,
                 int P, int64_t n_tiles, const double* w, double* out, double* lrec) {
    const bool lds_acc = gm.path == kMnGradCsrLds;
    const int apad = lds_acc ? ((gm.C1 * gm.d + 1) & ~1) : 0;
    int mb, waves;
    mn_wave_buffers(gm, 1, apad, &mb, &waves);
    const size_t lds = ((size_t)apad + (size_t)waves * mb) * sizeof(double);
    const unsigned blocks = persistent_blocks(n_tiles, waves, num_cus);
    if (lds_acc && !gm.wide)
        return launch_lds(grad_mn_csr<S, true, true>, blocks, waves * 64, lds, st, descs, tile0, P, n_tiles, gm, w, mb, apad, out, lrec);
    if (lds_acc)
        return launch_lds(grad_mn_csr<S, true, false>, blocks, waves * 64, lds, st, descs, tile0, P, n_tiles, gm, w, mb, apad, out, lrec);
    if (!gm.wide)
        return launch_lds(grad_mn_csr<S, false, true>, blocks, waves * 64, lds, st, descs, tile0, P, n_tiles, gm, w, mb, apad, out, lrec);
    return launch_lds(grad_mn_csr<S, false, false>, blocks, waves * 64, lds, st, descs, tile0, P, n_tiles, gm, w, mb, apad, out, lrec);
}

int64_t merged_spans(int64_t T) {
    const int64_t s = grad_merge_span(T);
    return (T + s - 1) / s;
}

// The scratch: [rec: n x C1 d | rec2 | lrec: T x 2 | lrec2 | mult].
struct MnScratch {
    int64_t n_rec;
    size_t rec2, lrec, lrec2, mult, total;
};
MnScratch mn_scratch(const MnGradGeom& gm, int64_t n_tiles) {
    MnScratch s{};
    const int64_t T = std::max<int64_t>(n_tiles, 1);
    const size_t Wg = (size_t)gm.C1 * (size_t)gm.d;
    s.n_rec = gm.path == kMnGradFused ? T : gm.path == kMnGradGeneral ? (T + gm.span - 1) / gm.span : 0;
    s.rec2 = (size_t)s.n_rec * Wg;
    s.lrec = s.rec2 + (s.n_rec ? (size_t)merged_spans(s.n_rec) * Wg : 0);
    s.lrec2 = s.lrec + 2 * (size_t)T;
    s.mult = s.lrec2 + 2 * (size_t)merged_spans(T);
    s.total = s.mult + (gm.path == kMnGradGeneral
                            ? (size_t)std::min<int64_t>(gm.range, T) * (size_t)gm.tile_rows * (size_t)gm.C1
                            : 0);
    return s;
}

bool env_set(const char* name) {
    const char* e = getenv(name);
    return e && *e && *e != '0';
}

int pow2_at_least(int64_t n) {
    int p = 1;
    while (p < n) p *= 2;
    return p;
}

}  // namespace

// PSGD_GRAD_MN_TWO_PASS=1 (tests, A/B): a dense shape that would run fused takes the general path.
// Read at every call, like PSGD_GRAD_CSR_GLOBAL.
MnGradGeom grad_mn_geometry(int layout, int storage, int d, int num_classes, int64_t max_nnz) {
    MnGradGeom gm{};
    gm.d = d;
    gm.C1 = num_classes - 1;
    gm.tile_rows = stats_geometry(layout, d, storage).tile_rows;
    gm.wide = gm.C1 > kMnLaneClasses ? 1 : 0;
    gm.span = 1;
    if (layout == kCsr) {
        gm.group = max_nnz <= 16 ? 16 : max_nnz <= 32 ? 32 : 64;
        const int64_t cells = (int64_t)gm.C1 * d;
        gm.path = grad_csr_lds_applies((int)std::min<int64_t>(cells, INT32_MAX)) ? kMnGradCsrLds : kMnGradCsrGlobal;
        return gm;
    }
    const int vec = storage == 1 ? 4 : 2;
    gm.nvec = (d + vec - 1) / vec;
    // the fused kernel's geometry is grad_dense's
    const int gl = gm.nvec < 64 ? pow2_at_least(gm.nvec) : 64;
    const int nvl = pow2_at_least((gm.nvec + gl - 1) / gl);
    const int cp = std::max(2, pow2_at_least(gm.C1));
    const bool fits = gm.C1 <= kGmFusedClasses && (int64_t)nvl * cp <= kGmFusedVecs;
    // where the fused kernel beat the general path on the same rows (tools/grad_mn_bench.py --what
    // sweep): narrow rows (at most 16 lanes a row) at any K <= 17; K = 3 at any d;
    // K = 4, 5 except rows of 33 .. 64 vectors (64 lanes with one vector each: the most reduction
    // steps a byte). PSGD_GRAD_MN_FUSE_ALL=1 (A/B) fuses whatever fits the registers.
    const bool wins = gl <= 16 || cp == 2 || (cp == 4 && !(gl == 64 && nvl == 1));
    if (fits && (wins || env_set("PSGD_GRAD_MN_FUSE_ALL")) && !env_set("PSGD_GRAD_MN_TWO_PASS")) {
        gm.path = kMnGradFused;
        gm.group = gl;
        gm.nvl = nvl;
        gm.cp = cp;
        gm.wlds = 1;
        return gm;
    }
    gm.path = kMnGradGeneral;
    const int xh = kMnHold / vec;
    gm.group = std::min(64, pow2_at_least((gm.nvec + xh - 1) / xh));
    gm.wlds = (int64_t)gm.C1 * mn_lds_pitch(d, storage) <= kMnWLds ? 1 : 0;
    gm.agroup = std::min(64, pow2_at_least((gm.nvec + kGmChunkVecs - 1) / kGmChunkVecs));
    gm.n_colchunks = (gm.nvec + gm.agroup * kGmChunkVecs - 1) / (gm.agroup * kGmChunkVecs);
    const int per_item = (64 / gm.agroup) * kGmChunkClasses;
    gm.n_classchunks = (gm.C1 + per_item - 1) / per_item;
    gm.span = pow2_at_least((gm.C1 + 15) / 16);
    int64_t range = 1;
    while (2 * range * gm.tile_rows * gm.C1 <= kGmMultDoubles && range < (1 << 30)) range *= 2;
    // PSGD_GRAD_MN_RANGE=n (tests): at most n tiles a range, so that a small batch takes several
    if (const char* e = getenv("PSGD_GRAD_MN_RANGE")) {
        const long cap = atol(e);
        while (cap >= 1 && range > cap) range /= 2;
    }
    gm.range = (int32_t)range;
    return gm;
}

size_t grad_mn_scratch(const MnGradGeom& gm, int64_t n_tiles) { return mn_scratch(gm, n_tiles).total; }

int launch_gradient_mn(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                       const MnGradGeom& gm, int storage, const double* w, double* scratch, double* out,
                       int num_cus, hipStream_t st) {
    const size_t Wg = (size_t)gm.C1 * (size_t)gm.d;
    const bool csr = gm.path == kMnGradCsrLds || gm.path == kMnGradCsrGlobal;
    if (n_tiles <= 0 || csr) {
        const int e = (int)hipMemsetAsync(out, 0, (Wg + 2) * sizeof(double), st);
        if (e || n_tiles <= 0) return e;
    }
    const MnScratch s = mn_scratch(gm, n_tiles);
    double* rec = scratch;
    double* lrec = scratch + s.lrec;
    int e;
    if (csr)
        e = storage == 1 ? launch_csr_s<float>(gm, num_cus, st, descs, tile0, n_parts, n_tiles, w, out, lrec)
                         : launch_csr_s<double>(gm, num_cus, st, descs, tile0, n_parts, n_tiles, w, out, lrec);
    else if (gm.path == kMnGradFused)
        e = storage == 1 ? launch_fused_s<float>(gm, num_cus, st, descs, tile0, n_parts, n_tiles, w, rec, lrec)
                         : launch_fused_s<double>(gm, num_cus, st, descs, tile0, n_parts, n_tiles, w, rec, lrec);
    else
        e = storage == 1 ? launch_general_s<float>(gm, num_cus, st, descs, tile0, n_parts, n_tiles, w, rec, lrec, scratch + s.mult)
                         : launch_general_s<double>(gm, num_cus, st, descs, tile0, n_parts, n_tiles, w, rec, lrec, scratch + s.mult);
    if (e) return e;
    if (!csr) {
        e = grad_merge_records(rec, s.n_rec, (int64_t)Wg, scratch + s.rec2, out, st);
        if (e) return e;
    }
    return grad_merge_records(lrec, n_tiles, 2, scratch + s.lrec2, out + Wg, st);
}

}  // namespace psgd
