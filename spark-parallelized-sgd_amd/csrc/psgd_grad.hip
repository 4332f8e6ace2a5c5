// psgd_grad.hip -- the batch gradient at fixed weights over the registered partitions
// (psgd_gradient_sum) and MLlib's stateless updaters applied to it (psgd_gd_update): what MLlib
// 1.6.1's GradientDescent.runMiniBatchSGD computes per iteration inside treeAggregate
// (gradientSum[j] = sum_i mult_i x_ij, lossSum = sum_i loss_i, count; (loss_i, mult_i) =
// gradient_scalar<GRAD, double>(x_i . w, y_i)), in fp64 whatever the storage.
//
// No chain, as in psgd_eval.hip / psgd_colstats.hip: the batch is cut into the statistics passes'
// tiles (tile0[p] is partition p's first tile, numbered across the partitions in partition-index
// order). A sampled batch (ChainDesc::rows non-null) keeps the tiling of the whole partition: tile t
// holds samples [t tile_rows, (t + 1) tile_rows) of the batch, and the tiles past the batch's end
// give zero records -- the tiling never depends on a count that only the device knows.
//
// Dense rows, fused, bitwise reproducible: a work item is a tile. Lanes lie across a row's 16-byte
// vectors (lane j of a group of gl takes vectors j, j + gl, ..: NVL of them cover the row), so a
// lane owns fixed columns and keeps their fp64 accumulators in registers for the whole tile. A wave
// holds up to 64 rows' vectors in registers at a time (R rows a lane group, 64 / gl groups): their
// partial dots against the weights (LDS, f64) are group_sum'ed and parked in LDS, lane i evaluates
// row i's multiplier and loss (one exp a row, not one a lane), and every lane then adds mult . x
// into its accumulators from the registers that still hold the rows. A tile ends with one record of
// d doubles + {loss, count}; grad_merge adds the records in tile order -- spans of consecutive tiles
// first, then the spans in order. No floating-point atomics: the same bits from call to call and
// for any grid size. Rows wider than 512 vectors (d > 2,048 f32, d > 1,024 f64) take two passes
// with the same records: grad_rowmult writes every row's multiplier (and the tile's loss),
// grad_wsum adds mult . x per (tile, column chunk) in stats_dense's layout.
//
// CSR rows, gradientSum NOT bitwise reproducible: columns scatter over up to 2^22 features. One
// pass: a wave takes 64 rows at a time -- dots by gather of w[col], the multipliers with one row a
// lane, then the rows again (from cache) adding mult . val into the output with fp64 vector atomics.
// Narrow models (8 d bytes fit the workgroup's LDS budget) accumulate in an fp64 vector in LDS with
// LDS adds and flush it once a workgroup with contiguous global adds. lossSum and count are
// per-tile sums merged in tile order: reproducible.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include <cstdlib>

#include "psgd_device.h"
#include "psgd_eval.h"

namespace psgd {
namespace {

constexpr int kGradBlock = 256;
constexpr int kGradWaves = kGradBlock / 64;
constexpr int kGradMaxNvl = 8;       // fused: at most this many 16-byte vectors of a row a lane
constexpr int kGradChunkVecs = 2;    // two-pass: vectors a lane owns of a column chunk (stats_dense's)
constexpr int kGradLdsFeatures = 6144;   // CSR: fp64 accumulators a workgroup keeps in LDS (48 KiB)

// buf[0 .. n) holds the dots of batch rows row0 .. row0 + n (n <= 64): lane i < n replaces dot i by
// row i's multiplier and adds its loss to loss_acc; rows at or past r1 get multiplier 0.
template <int GRAD>
__device__ __forceinline__ void eval_rows(double* buf, int n, const double* __restrict__ y, int64_t row0,
                                          int64_t r1, int lane, double& loss_acc) {
    wave_lds_sync();
    if (lane < n) {
        double mult = 0.0;
        if (row0 + lane < r1) {
            const double loss = gradient_scalar<GRAD, double>(buf[lane], y[row0 + lane], mult);
            loss_acc += loss;
        }
        buf[lane] = mult;
    }
    wave_lds_sync();
}

// Narrow rows (NVL <= 2) keep two sets of row registers, the next round's loads in flight under this
// round's arithmetic; wider rows have the registers for one set only (a second costs a wave a SIMD).
template <int NVL>
constexpr bool fused_pipelined() { return NVL <= 2; }
// Rows of a lane group in one set of row registers: 8 to 16 vectors a lane.
template <int NVL>
constexpr int fused_rows() { return NVL >= 8 ? 2 : 4; }

// (two workgroups a CU up to NVL = 4: the row registers and accumulators fit 256 VGPRs)
template <typename S, int GRAD, int NVL>
__global__ __launch_bounds__(kGradBlock, NVL <= 4 ? 2 : 1) void grad_dense(const ChainDesc* __restrict__ descs,
                                                         const int64_t* __restrict__ tile0, int P,
                                                         int64_t n_tiles, GradGeom gm,
                                                         const double* __restrict__ w, double* __restrict__ rec) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int R = fused_rows<NVL>();
    extern __shared__ __attribute__((aligned(16))) double w_lds[];   // gl * NVL * VEC, zero past d
    __shared__ double park[kGradWaves][64];
    const int d = gm.d;
    const int gl = gm.group, rpw = 64 / gl;
    for (int i = threadIdx.x; i < gl * NVL * VEC; i += kGradBlock) w_lds[i] = i < d ? w[i] : 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g = lane / gl, j = lane & (gl - 1);
    // rows a group holds at a time: the wave's rows of one round are at most 64 (one a lane)
    const int ract = R < gl ? R : gl;
    const int round = rpw * ract;
    const int nfull = d / VEC, rem = d - nfull * VEC;
    // the lane's vectors; one past the row's last reads vector 0 instead (times weights of 0.0)
    int vc[NVL];
    bool vok[NVL];
#pragma unroll
    for (int u = 0; u < NVL; ++u) {
        const int v = u * gl + j;
        vok[u] = v < gm.nvec;
        vc[u] = vok[u] ? v : 0;
    }
    const int u_part = rem ? nfull / gl : -1;   // the row's partial vector is vector u_part of lane nfull % gl
    double* buf = park[wave];
    const int64_t W = (int64_t)d + 2;
    for (int64_t tile = (int64_t)blockIdx.x * kGradWaves + wave; tile < n_tiles;
         tile += (int64_t)gridDim.x * kGradWaves) {
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        double G[NVL][VEC];
#pragma unroll
        for (int u = 0; u < NVL; ++u)
#pragma unroll
            for (int e = 0; e < VEC; ++e) G[u][e] = 0.0;
        double loss_acc = 0.0;
        auto load = [&](V (&xv)[R][NVL], int64_t rb) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < R; ++q) {
                if (q < ract) {
                    const int64_t r = rb + (int64_t)q * rpw + g;
                    // (a lane group past the tile's end re-reads its first row; its multiplier is 0)
                    const int64_t rr = r < r1 ? r : r0;
                    const int64_t ri = dsc.rows ? (int64_t)dsc.rows[rr] : rr;
                    const V* row = reinterpret_cast<const V*>(X + ri * dsc.ld);
#pragma unroll
                    for (int u = 0; u < NVL; ++u) xv[q][u] = __builtin_nontemporal_load(as_global(row + vc[u]));
                }
            }
        };
        // (the rows stay in registers as stored; they are widened once for the dot and once for the
        // accumulators: f64 copies of the f32 vectors would double their registers)
        auto widen = [&](const V& v, int u, double* x) __attribute__((always_inline)) {
            unpack<S, double>(v, x);
            if (u == u_part) {
                // the pad of the partial vector is the caller's (zero-copy rows): not used
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (vc[u] == nfull && e >= rem) x[e] = 0.0;
            }
        };
        auto compute = [&](const V (&xv)[R][NVL], int64_t rb) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < R; ++q) {
                if (q < ract) {
                    double acc = 0.0;
#pragma unroll
                    for (int u = 0; u < NVL; ++u) {
                        double x[VEC];
                        widen(xv[q][u], u, x);
                        // (a vector past the row's last meets weights of 0.0)
#pragma unroll
                        for (int e = 0; e < VEC; ++e)
                            acc = __builtin_fma(x[e], w_lds[(u * gl + j) * VEC + e], acc);
                    }
                    const double dot = group_sum(acc, gl);
                    if (j == 0) buf[q * rpw + g] = dot;
                }
            }
            eval_rows<GRAD>(buf, round, dsc.y, rb, r1, lane, loss_acc);
#pragma unroll
            for (int q = 0; q < R; ++q) {
                if (q < ract) {
                    const double m = buf[q * rpw + g];
#pragma unroll
                    for (int u = 0; u < NVL; ++u) {
                        double x[VEC];
                        widen(xv[q][u], u, x);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) G[u][e] = __builtin_fma(m, x[e], G[u][e]);
                    }
                }
            }
            wave_lds_sync();   // the next round's dots overwrite the multipliers
        };
        if constexpr (fused_pipelined<NVL>()) {
            V xa[R][NVL], xb[R][NVL];
            int64_t rb = r0;
            if (rb < r1) load(xa, rb);
            while (rb < r1) {
                if (rb + round < r1) load(xb, rb + round);
                compute(xa, rb);
                rb += round;
                if (rb >= r1) break;
                if (rb + round < r1) load(xa, rb + round);
                compute(xb, rb);
                rb += round;
            }
        } else {
            V xa[R][NVL];
            for (int64_t rb = r0; rb < r1; rb += round) {
                load(xa, rb);
                compute(xa, rb);
            }
        }
        // narrow rows: the wave's 64 / gl lane groups hold different rows of the same columns
        for (int m = gl; m < 64; m <<= 1) {
#pragma unroll
            for (int u = 0; u < NVL; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) G[u][e] += __shfl_xor(G[u][e], m, 64);
        }
        loss_acc = wave_sum(loss_acc);
        double* out = rec + tile * W;
        if (g == 0) {
#pragma unroll
            for (int u = 0; u < NVL; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int c = vc[u] * VEC + e;
                    if (vok[u] && c < d) out[c] = G[u][e];
                }
        }
        if (lane == 0) {
            out[d] = loss_acc;
            out[d + 1] = r1 > r0 ? (double)(r1 - r0) : 0.0;
        }
    }
}

// Two-pass path, pass 1: every row's multiplier into mult[tile * tile_rows + (r - r0)] and the
// tile's {loss, count} into its record. Rows of 64 lanes (more than 512 vectors), weights from L2.
template <typename S, int GRAD>
__global__ __launch_bounds__(kGradBlock) void grad_rowmult(const ChainDesc* __restrict__ descs,
                                                           const int64_t* __restrict__ tile0, int P,
                                                           int64_t n_tiles, GradGeom gm,
                                                           const double* __restrict__ w, double* __restrict__ mult,
                                                           double* __restrict__ rec) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int R = 4;
    __shared__ double park[kGradWaves][64];
    const int d = gm.d;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nfull = d / VEC, rem = d - nfull * VEC;
    double* buf = park[wave];
    const int64_t W = (int64_t)d + 2;
    for (int64_t tile = (int64_t)blockIdx.x * kGradWaves + wave; tile < n_tiles;
         tile += (int64_t)gridDim.x * kGradWaves) {
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        double* mt = mult + tile * gm.tile_rows;
        double loss_acc = 0.0;
        // 64 rows a round: R at a time, their dots parked for eval_rows
        for (int64_t rb = r0; rb < r1; rb += 64) {
            for (int qb = 0; qb < 64 && rb + qb < r1; qb += R) {
                const V* row[R];
                double acc[R];
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const int64_t r = rb + qb + q;
                    const int64_t rr = r < r1 ? r : r0;
                    const int64_t ri = dsc.rows ? (int64_t)dsc.rows[rr] : rr;
                    row[q] = reinterpret_cast<const V*>(X + ri * dsc.ld);
                    acc[q] = 0.0;
                }
                for (int v = lane; v < gm.nvec; v += 64) {
                    V xv[R];
#pragma unroll
                    for (int q = 0; q < R; ++q) xv[q] = __builtin_nontemporal_load(as_global(row[q] + v));
                    double wv[VEC];
#pragma unroll
                    for (int e = 0; e < VEC; ++e) wv[e] = v * VEC + e < d ? w[v * VEC + e] : 0.0;
#pragma unroll
                    for (int q = 0; q < R; ++q) {
                        double x[VEC];
                        unpack<S, double>(xv[q], x);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            if (rem && v == nfull && e >= rem) x[e] = 0.0;
                            acc[q] = __builtin_fma(x[e], wv[e], acc[q]);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const double dot = wave_sum(acc[q]);
                    if (lane == 0) buf[qb + q] = dot;
                }
            }
            eval_rows<GRAD>(buf, 64, dsc.y, rb, r1, lane, loss_acc);
            if (rb + lane < r1) mt[rb - r0 + lane] = buf[lane];
            wave_lds_sync();
        }
        loss_acc = wave_sum(loss_acc);
        if (lane == 0) {
            rec[tile * W + d] = loss_acc;
            rec[tile * W + d + 1] = r1 > r0 ? (double)(r1 - r0) : 0.0;
        }
    }
}

// Two-pass path, pass 2: a work item is (tile, column chunk of 64 * kGradChunkVecs vectors); the
// lane's columns' sums of mult . x over the tile's rows, in row order, into the tile's record.
template <typename S>
__global__ __launch_bounds__(kGradBlock) void grad_wsum(const ChainDesc* __restrict__ descs,
                                                        const int64_t* __restrict__ tile0, int P,
                                                        int64_t n_items, GradGeom gm,
                                                        const double* __restrict__ mult, double* __restrict__ rec) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int U = kGradChunkVecs, R = 4;
    const int d = gm.d;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t W = (int64_t)d + 2;
    for (int64_t item = (int64_t)blockIdx.x * kGradWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kGradWaves) {
        const int64_t tile = item / gm.n_chunks;
        const int chunk = (int)(item - tile * gm.n_chunks);
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        const double* mt = mult + tile * gm.tile_rows;
        int v[U], vc[U];
        bool vok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v[u] = (chunk * U + u) * 64 + lane;
            vok[u] = v[u] < gm.nvec;
            vc[u] = vok[u] ? v[u] : 0;
        }
        double G[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < VEC; ++e) G[u][e] = 0.0;
        for (int64_t rb = r0; rb < r1; rb += R) {
            V xv[R][U];
            double m[R];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const int64_t r = rb + q;
                const int64_t rr = r < r1 ? r : r0;
                const int64_t ri = dsc.rows ? (int64_t)dsc.rows[rr] : rr;
                const V* row = reinterpret_cast<const V*>(X + ri * dsc.ld);
                m[q] = r < r1 ? mt[r - r0] : 0.0;
#pragma unroll
                for (int u = 0; u < U; ++u) xv[q][u] = __builtin_nontemporal_load(as_global(row + vc[u]));
            }
#pragma unroll
            for (int q = 0; q < R; ++q)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    double x[VEC];
                    unpack<S, double>(xv[q][u], x);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        // (columns at or past d are never written; their values may be anything)
                        const double xe = vc[u] * VEC + e < d ? x[e] : 0.0;
                        G[u][e] = __builtin_fma(m[q], xe, G[u][e]);
                    }
                }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int c = v[u] * VEC + e;
                if (vok[u] && c < d) rec[tile * W + c] = G[u][e];
            }
    }
}

// Records [T][W]: thread (column, span) adds records [span * s, span * (s + 1)) in order into dst[s].
__global__ __launch_bounds__(kGradBlock) void grad_merge(const double* __restrict__ src, int64_t T, int64_t span,
                                                         double* __restrict__ dst, int64_t W, int64_t dst_stride) {
    const int64_t c = (int64_t)blockIdx.x * kGradBlock + threadIdx.x;
    const int64_t s = blockIdx.y;
    if (c >= W) return;
    const int64_t t0 = s * span, t1 = t0 + span < T ? t0 + span : T;
    double a = 0.0;
    for (int64_t t = t0; t < t1; ++t) a += src[t * W + c];
    dst[s * dst_stride + c] = a;
}

// ---- CSR ----
__device__ __forceinline__ void lds_add(double* p, double v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// LDSACC: the workgroup's accumulator of d doubles lives in LDS and is flushed once at the end.
template <typename S, int GRAD, bool LDSACC>
__global__ __launch_bounds__(kGradBlock) void grad_csr(const ChainDesc* __restrict__ descs,
                                                       const int64_t* __restrict__ tile0, int P,
                                                       int64_t n_tiles, GradGeom gm, const double* __restrict__ w,
                                                       double* out, double* __restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) double acc_lds[];
    __shared__ double park[kGradWaves][64];
    const int d = gm.d;
    if constexpr (LDSACC) {
        for (int i = threadIdx.x; i < d; i += kGradBlock) acc_lds[i] = 0.0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gl = gm.group, rpw = 64 / gl;
    const int g = lane / gl, j = lane & (gl - 1);
    double* buf = park[wave];
    for (int64_t tile = (int64_t)blockIdx.x * kGradWaves + wave; tile < n_tiles;
         tile += (int64_t)gridDim.x * kGradWaves) {
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        const S* val = reinterpret_cast<const S*>(dsc.x);
        double loss_acc = 0.0;
        for (int64_t rb = r0; rb < r1; rb += 64) {
            // the dots of rows rb .. rb + 64, one row a lane group at a time
            for (int qb = 0; qb < 64; qb += rpw) {
                const int64_t r = rb + qb + g;
                const bool valid = r < r1;
                double a = 0.0;
                if (valid) {
                    const int64_t ri = dsc.rows ? (int64_t)dsc.rows[r] : r;
                    const int64_t e = dsc.row_ptr[ri + 1];
                    for (int64_t k = dsc.row_ptr[ri] + j; k < e; k += gl)
                        a = __builtin_fma((double)val[k], w[dsc.col[k]], a);
                }
                const double dot = group_sum(a, gl);
                if (j == 0) buf[qb + g] = dot;
            }
            eval_rows<GRAD>(buf, 64, dsc.y, rb, r1, lane, loss_acc);
            // the same rows again (from cache): mult . val into the accumulator
            for (int qb = 0; qb < 64; qb += rpw) {
                const int64_t r = rb + qb + g;
                if (r < r1) {
                    const double m = buf[qb + g];
                    if (m != 0.0) {
                        const int64_t ri = dsc.rows ? (int64_t)dsc.rows[r] : r;
                        const int64_t e = dsc.row_ptr[ri + 1];
                        for (int64_t k = dsc.row_ptr[ri] + j; k < e; k += gl) {
                            const double t = m * (double)val[k];
                            const int c = dsc.col[k];
                            if constexpr (LDSACC) lds_add(acc_lds + c, t); else unsafeAtomicAdd(out + c, t);
                        }
                    }
                }
            }
            wave_lds_sync();
        }
        loss_acc = wave_sum(loss_acc);
        if (lane == 0) {
            rec[2 * tile] = loss_acc;
            rec[2 * tile + 1] = r1 > r0 ? (double)(r1 - r0) : 0.0;
        }
    }
    if constexpr (LDSACC) {
        __syncthreads();
        // 64 consecutive doubles a wave instruction: 512 contiguous bytes of atomics
        for (int i = threadIdx.x; i < d; i += kGradBlock) {
            const double v = acc_lds[i];
            if (v != 0.0) unsafeAtomicAdd(out + i, v);
        }
    }
}

// ---- Update ----
constexpr int kUpdPerBlock = 1024;   // elements a workgroup updates: thread t takes t, t + 256, ..

// w_out = updater.compute(w, sum[0 .. d) / sum[d + 1], stepSize, iter, regParam)._1 with s =
// stepSize / sqrt(iter); part[block] = the block's share of ||w_out||^2 (SquaredL2) or ||w_out||_1
// (L1), summed in an order the geometry fixes.
template <int UPD>
__global__ __launch_bounds__(kGradBlock) void gd_update(int d, const double* w, const double* __restrict__ sum,
                                                        double s, double reg, double* w_out,
                                                        double* __restrict__ part) {
    __shared__ double sh[kGradWaves];
    const double n = sum[d + 1];
    double acc = 0.0;
    for (int k = 0; k < kUpdPerBlock / kGradBlock; ++k) {
        const int64_t i = (int64_t)blockIdx.x * kUpdPerBlock + k * kGradBlock + threadIdx.x;
        if (i >= d) break;
        const double g = sum[i] / n;
        double t = w[i];
        if constexpr (UPD == U_SQUARED_L2) t = t * (1.0 - s * reg);   // UPD.scala:172-174
        t = t + (-s) * g;                                            // axpy(-thisIterStepSize, gradient, w)
        if constexpr (UPD == U_L1) {                                 // UPD.scala:136-143
            const double shrink = reg * s;
            t = jsignum(t) * jmax(0.0, m_fabs(t) - shrink);
        }
        w_out[i] = t;
        if constexpr (UPD == U_SQUARED_L2) acc = acc + t * t;
        if constexpr (UPD == U_L1) acc = acc + m_fabs(t);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// regval = 0 (Simple), 0.5 reg ||w'||^2 (SquaredL2), reg ||w'||_1 (L1): one wave adds the blocks'
// shares, lane l blocks l, l + 64, .. in order, then one butterfly.
template <int UPD>
__global__ __launch_bounds__(64) void gd_regval(const double* __restrict__ part, int n_blocks, double reg,
                                                double* __restrict__ regval) {
    double a = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += 64) a += part[b];
    a = wave_sum(a);
    if (threadIdx.x == 0) {
        if constexpr (UPD == U_SQUARED_L2) {
            const double nrm = sqrt(a);
            *regval = 0.5 * reg * nrm * nrm;
        } else if constexpr (UPD == U_L1) {
            *regval = a * reg;
        } else {
            *regval = 0.0;
        }
    }
}

unsigned column_blocks(int64_t n) { return (unsigned)((n + kGradBlock - 1) / kGradBlock); }

template <typename S, int GRAD>
int launch_fused(const GradGeom& gm, unsigned blocks, hipStream_t st, const ChainDesc* descs, const int64_t* tile0,
                 int P, int64_t n_tiles, const double* w, double* rec) {
    constexpr int VEC = Vec16<S>::N;
    const size_t lds = (size_t)gm.group * gm.nvl * VEC * sizeof(double);
    const dim3 gr(blocks), bl(kGradBlock);
    switch (gm.nvl) {
        case 1: hipLaunchKernelGGL((grad_dense<S, GRAD, 1>), gr, bl, lds, st, descs, tile0, P, n_tiles, gm, w, rec); break;
        case 2: hipLaunchKernelGGL((grad_dense<S, GRAD, 2>), gr, bl, lds, st, descs, tile0, P, n_tiles, gm, w, rec); break;
        case 4: hipLaunchKernelGGL((grad_dense<S, GRAD, 4>), gr, bl, lds, st, descs, tile0, P, n_tiles, gm, w, rec); break;
        case 8: hipLaunchKernelGGL((grad_dense<S, GRAD, 8>), gr, bl, lds, st, descs, tile0, P, n_tiles, gm, w, rec); break;
        default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

template <typename S, int GRAD>
int launch_dense_sg(const GradGeom& gm, int num_cus, hipStream_t st, const ChainDesc* descs, const int64_t* tile0,
                    int P, int64_t n_tiles, const double* w, double* rec, double* mult) {
    // (the fused kernel's accumulators and rows in flight leave room for two workgroups a CU)
    if (gm.fused) return launch_fused<S, GRAD>(gm, grad_balanced_blocks(n_tiles, num_cus, 2), st, descs, tile0, P, n_tiles, w, rec);
    hipLaunchKernelGGL((grad_rowmult<S, GRAD>), dim3(grad_balanced_blocks(n_tiles, num_cus, 8)), dim3(kGradBlock), 0, st,
                       descs, tile0, P, n_tiles, gm, w, mult, rec);
    int e = (int)hipGetLastError();
    if (e) return e;
    const int64_t n_items = n_tiles * gm.n_chunks;
    hipLaunchKernelGGL(grad_wsum<S>, dim3(grad_balanced_blocks(n_items, num_cus, 8)), dim3(kGradBlock), 0, st, descs, tile0,
                       P, n_items, gm, mult, rec);
    return (int)hipGetLastError();
}

template <typename S>
int launch_dense_s(int gradient, const GradGeom& gm, int num_cus, hipStream_t st, const ChainDesc* descs,
                   const int64_t* tile0, int P, int64_t n_tiles, const double* w, double* rec, double* mult) {
    switch (gradient) {
        case G_LOGISTIC: return launch_dense_sg<S, G_LOGISTIC>(gm, num_cus, st, descs, tile0, P, n_tiles, w, rec, mult);
        case G_LEAST_SQUARES: return launch_dense_sg<S, G_LEAST_SQUARES>(gm, num_cus, st, descs, tile0, P, n_tiles, w, rec, mult);
        case G_HINGE: return launch_dense_sg<S, G_HINGE>(gm, num_cus, st, descs, tile0, P, n_tiles, w, rec, mult);
    }
    return -2;
}

template <typename S, int GRAD>
int launch_csr_sg(const GradGeom& gm, bool lds, unsigned blocks, hipStream_t st, const ChainDesc* descs,
                  const int64_t* tile0, int P, int64_t n_tiles, const double* w, double* out, double* rec) {
    if (lds)
        hipLaunchKernelGGL((grad_csr<S, GRAD, true>), dim3(blocks), dim3(kGradBlock), (size_t)gm.d * sizeof(double), st,
                           descs, tile0, P, n_tiles, gm, w, out, rec);
    else
        hipLaunchKernelGGL((grad_csr<S, GRAD, false>), dim3(blocks), dim3(kGradBlock), 0, st, descs, tile0, P, n_tiles,
                           gm, w, out, rec);
    return (int)hipGetLastError();
}

template <typename S>
int launch_csr_s(int gradient, const GradGeom& gm, bool lds, unsigned blocks, hipStream_t st, const ChainDesc* descs,
                 const int64_t* tile0, int P, int64_t n_tiles, const double* w, double* out, double* rec) {
    switch (gradient) {
        case G_LOGISTIC: return launch_csr_sg<S, G_LOGISTIC>(gm, lds, blocks, st, descs, tile0, P, n_tiles, w, out, rec);
        case G_LEAST_SQUARES: return launch_csr_sg<S, G_LEAST_SQUARES>(gm, lds, blocks, st, descs, tile0, P, n_tiles, w, out, rec);
        case G_HINGE: return launch_csr_sg<S, G_HINGE>(gm, lds, blocks, st, descs, tile0, P, n_tiles, w, out, rec);
    }
    return -2;
}

}  // namespace

unsigned grad_balanced_blocks(int64_t n_items, int num_cus, int per_cu) {
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * per_cu * kGradWaves;
    const int64_t rounds = (n_items + cap - 1) / cap;
    const int64_t waves = (n_items + rounds - 1) / rounds;
    return (unsigned)((waves + kGradWaves - 1) / kGradWaves);
}

// records [T][W] -> dst[W] in two levels (rec2: [n_spans][W])
int grad_merge_records(const double* rec, int64_t T, int64_t W, double* rec2, double* dst, hipStream_t st) {
    const int64_t span = grad_merge_span(T);
    const int64_t n_spans = (T + span - 1) / span;
    hipLaunchKernelGGL(grad_merge, dim3(column_blocks(W), (unsigned)n_spans), dim3(kGradBlock), 0, st, rec, T, span,
                       rec2, W, W);
    int e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(grad_merge, dim3(column_blocks(W), 1), dim3(kGradBlock), 0, st, rec2, n_spans, n_spans, dst, W, W);
    return (int)hipGetLastError();
}

GradGeom grad_geometry(int layout, int d, int storage, int64_t max_nnz, int tile_rows) {
    GradGeom gm{};
    gm.d = d;
    gm.tile_rows = tile_rows;
    if (layout == kCsr) {
        gm.group = max_nnz <= 16 ? 16 : max_nnz <= 32 ? 32 : 64;
        gm.n_chunks = 1;
        return gm;
    }
    const int vec = storage == 1 ? 4 : 2;
    gm.nvec = (d + vec - 1) / vec;
    int gl = 64;
    if (gm.nvec < 64) {
        gl = 1;
        while (gl < gm.nvec) gl *= 2;
    }
    gm.group = gl;
    const int need = (gm.nvec + gl - 1) / gl;
    int nvl = 1;
    while (nvl < need) nvl *= 2;
    gm.nvl = nvl;
    gm.fused = nvl <= kGradMaxNvl ? 1 : 0;
    gm.n_chunks = (gm.nvec + 64 * kGradChunkVecs - 1) / (64 * kGradChunkVecs);
    return gm;
}

int64_t grad_merge_span(int64_t n_tiles) {
    int64_t s = 32;
    while (s * s < n_tiles) ++s;
    return s;
}

// PSGD_GRAD_CSR_GLOBAL=1 (tests, A/B): narrow CSR models keep the global-atomic path. Read at every
// call, like PSGD_PER_SAMPLE, so that one process can compare the two paths.
bool grad_csr_lds_applies(int d) {
    const char* e = getenv("PSGD_GRAD_CSR_GLOBAL");
    const bool forced_global = e && *e && *e != '0';
    return !forced_global && d <= kGradLdsFeatures;
}

int launch_gradient_dense(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                          const GradGeom& gm, int storage, int gradient, const double* w, double* rec, double* rec2,
                          double* mult, double* out, int num_cus, hipStream_t st) {
    if (gradient < G_LOGISTIC || gradient > G_HINGE) return -2;
    if (n_tiles <= 0) return (int)hipMemsetAsync(out, 0, ((size_t)gm.d + 2) * sizeof(double), st);
    const int e = storage == 1 ? launch_dense_s<float>(gradient, gm, num_cus, st, descs, tile0, n_parts, n_tiles, w, rec, mult)
                               : launch_dense_s<double>(gradient, gm, num_cus, st, descs, tile0, n_parts, n_tiles, w, rec, mult);
    if (e) return e;
    return grad_merge_records(rec, n_tiles, (int64_t)gm.d + 2, rec2, out, st);
}

int launch_gradient_csr(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                        const GradGeom& gm, int storage, int gradient, bool lds, const double* w, double* rec,
                        double* rec2, double* out, int num_cus, hipStream_t st) {
    if (gradient < G_LOGISTIC || gradient > G_HINGE) return -2;
    int e = (int)hipMemsetAsync(out, 0, ((size_t)gm.d + 2) * sizeof(double), st);
    if (e || n_tiles <= 0) return e;
    // LDS accumulators: 48 KiB a workgroup at most, so three workgroups a CU
    const unsigned blocks = grad_balanced_blocks(n_tiles, num_cus, lds ? 2 : 8);
    e = storage == 1 ? launch_csr_s<float>(gradient, gm, lds, blocks, st, descs, tile0, n_parts, n_tiles, w, out, rec)
                     : launch_csr_s<double>(gradient, gm, lds, blocks, st, descs, tile0, n_parts, n_tiles, w, out, rec);
    if (e) return e;
    return grad_merge_records(rec, n_tiles, 2, rec2, out + gm.d, st);
}

int64_t gd_update_blocks(int d) { return ((int64_t)d + kUpdPerBlock - 1) / kUpdPerBlock; }

int launch_gd_update(int updater, int d, const double* w, const double* sum, double s, double reg, double* w_out,
                     double* part, double* regval, hipStream_t st) {
    const unsigned nb = (unsigned)gd_update_blocks(d);
    const dim3 gr(nb), bl(kGradBlock);
    switch (updater) {
        case U_SIMPLE:
            hipLaunchKernelGGL(gd_update<U_SIMPLE>, gr, bl, 0, st, d, w, sum, s, reg, w_out, part);
            hipLaunchKernelGGL(gd_regval<U_SIMPLE>, dim3(1), dim3(64), 0, st, part, (int)nb, reg, regval);
            break;
        case U_SQUARED_L2:
            hipLaunchKernelGGL(gd_update<U_SQUARED_L2>, gr, bl, 0, st, d, w, sum, s, reg, w_out, part);
            hipLaunchKernelGGL(gd_regval<U_SQUARED_L2>, dim3(1), dim3(64), 0, st, part, (int)nb, reg, regval);
            break;
        case U_L1:
            hipLaunchKernelGGL(gd_update<U_L1>, gr, bl, 0, st, d, w, sum, s, reg, w_out, part);
            hipLaunchKernelGGL(gd_regval<U_L1>, dim3(1), dim3(64), 0, st, part, (int)nb, reg, regval);
            break;
        default:
            return -2;
    }
    return (int)hipGetLastError();
}

}  // namespace psgd
