// psgd_eval.hip -- fixed-weight scoring passes over the registered partitions (psgd_evaluate,
// psgd_predict): every row's dot x_r . w in fp64, its loss (gradient.compute(x, y, w)._2,
// PSGD.scala:254 at constant w) and MLlib's default-threshold prediction, summed per partition.
//
// No chain: every row is independent, so the work is cut into (partition, tile of tile_rows rows)
// items that the waves of a persistent grid take in turn -- a partition is not tied to a CU as a
// chain is. Determinism: a tile is summed by one wave in an order its geometry alone fixes (lane
// l scores and adds rows l, l + 64, ... of every 256, in order, then one butterfly over the lanes) into
// tile_loss[tile]; eval_reduce adds a partition's tiles in tile order and the partitions in
// partition-index order (the combiner's order, PSGD.scala:271-276). No floating-point atomics:
// a partition's sum is the same bits whatever the grid size and whatever else is registered.
#include "psgd_device.h"
#include "psgd_eval.h"

namespace psgd {
namespace {

constexpr int kEvalBlock = 256;
constexpr int kEvalWaves = kEvalBlock / 64;
constexpr int kEvalRows = 4;          // dense: rows a lane group keeps in flight
constexpr int kEvalWLds = 4096;       // dense: weights of up to this many features live in LDS
                                      // (32 KiB beside the waves' 8 KiB of dots: three workgroups a CU)
constexpr int kReduceBlock = 1024;

// Loss and MLlib's default-threshold prediction of one row from its dot (LogisticRegressionModel:
// sigmoid > 0.5, SVMModel: margin > 0.0 -- both dot > 0.0).
template <int GRAD>
__device__ __forceinline__ void score_row(double dot, double y, double& loss, double& ok) {
    double mult;
    loss = gradient_scalar<GRAD, double>(dot, y, mult);
    ok = 0.0;
    if constexpr (GRAD != G_LEAST_SQUARES) ok = ((dot > 0.0 ? 1.0 : 0.0) == y) ? 1.0 : 0.0;
}

// The loss math (exp and log1p for Logistic: some hundreds of f64 operations) is not paid per
// wave pass, where one lane of a group would carry it: a wave parks its rows' dots in a buffer of
// its own in LDS, and every kDotBuf rows (and at the tile's end) scores them with all lanes, row
// i of the buffer in lane i % 64 -- labels read and margins written coalesced. Lane l adds its rows
// l, l + 64, ... in order: fixed by the tile's geometry like everything else.
constexpr int kDotBuf = 256;
template <int GRAD>
__device__ __forceinline__ void score_buffer(const double* buf, int n, const double* __restrict__ y,
                                             int64_t row0, double* __restrict__ margins, int lane,
                                             double& loss_acc, double& ok_acc) {
    wave_lds_sync();
    for (int i = lane; i < n; i += 64) {
        const double dot = buf[i];
        double loss, ok;
        score_row<GRAD>(dot, y[row0 + i], loss, ok);
        loss_acc += loss;
        ok_acc += ok;
        if (margins) margins[row0 + i] = dot;
    }
    wave_lds_sync();
}

// Dense rows: lanes across a row's 16-byte vectors (lane j of a group takes vectors j, j + gl, ...),
// gl = 64 for rows of 1 KiB or more, else the power of two that covers the row, so that a wave
// instruction reads 64 / gl consecutive rows -- contiguous bytes either way. kEvalRows rows per
// group in flight. WLDS: the weights in LDS as f64 (d <= kEvalWLds), else read from HBM / L2.
template <typename S, int GRAD, bool WLDS>
__global__ __launch_bounds__(kEvalBlock) void score_dense(const ChainDesc* __restrict__ descs,
                                                          const EvalPart* __restrict__ ep, int P,
                                                          int64_t n_items, const double* __restrict__ w,
                                                          int d, double* __restrict__ tile_loss,
                                                          double* __restrict__ tile_ok,
                                                          double* __restrict__ margins) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int R = kEvalRows;
    extern __shared__ __attribute__((aligned(16))) double w_lds[];
    __shared__ double dots_sh[kEvalWaves][kDotBuf];
    if constexpr (WLDS) {
        for (int i = threadIdx.x; i < d; i += kEvalBlock) w_lds[i] = w[i];
        __syncthreads();
    }
    auto weight = [&](int c) __attribute__((always_inline)) -> double {
        if constexpr (WLDS) return w_lds[c]; else return w[c];
    };
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nfull = d / VEC;            // whole vectors of a row
    const int rem = d - nfull * VEC;      // features in the row's last, partial vector
    const int64_t base = ep[0].tile0;
    for (int64_t item = (int64_t)blockIdx.x * kEvalWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kEvalWaves) {
        const int p = item_partition(ep, P, item);
        const ChainDesc dsc = descs[p];
        const int gl = ep[p].group;
        const int rpw = 64 / gl;
        const int g = lane / gl, j = lane & (gl - 1);
        const int64_t r0 = (item - (ep[p].tile0 - base)) * ep[p].tile_rows;
        const int64_t r1 = r0 + ep[p].tile_rows < dsc.n_rows ? r0 + ep[p].tile_rows : dsc.n_rows;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        double* dots = dots_sh[wave];
        int64_t buf_row = r0;   // the partition row of dots[0]
        double loss_acc = 0.0, ok_acc = 0.0;
        for (int64_t rb = r0; rb < r1; rb += (int64_t)rpw * R) {
            double acc[R];
            const V* row[R];
            int64_t rr[R];
            bool valid[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int64_t r = rb + (int64_t)u * rpw + g;
                valid[u] = r < r1;
                rr[u] = valid[u] ? r : r0;   // (a lane group past the tile's end re-reads its first row)
                row[u] = reinterpret_cast<const V*>(X + rr[u] * dsc.ld);
                acc[u] = 0.0;
            }
            for (int v = j; v < nfull; v += gl) {
                V xv[R];
#pragma unroll
                for (int u = 0; u < R; ++u) xv[u] = __builtin_nontemporal_load(as_global(row[u] + v));
                double wv[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) wv[e] = weight(v * VEC + e);
#pragma unroll
                for (int u = 0; u < R; ++u) {
                    double x[VEC];
                    unpack<S, double>(xv[u], x);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[u] = __builtin_fma(x[e], wv[e], acc[u]);
                }
            }
            if (rem && j == (nfull & (gl - 1))) {
                // the partial vector lies inside the row's pitch (ld * sizeof(S) is a multiple of 16)
#pragma unroll
                for (int u = 0; u < R; ++u) {
                    double x[VEC];
                    unpack<S, double>(__builtin_nontemporal_load(as_global(row[u] + nfull)), x);
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
                        if (e < rem) acc[u] = __builtin_fma(x[e], weight(nfull * VEC + e), acc[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const double dot = group_sum(acc[u], gl);
                if (valid[u] && j == 0) dots[rr[u] - buf_row] = dot;
            }
            // (rpw * R divides kDotBuf: the buffer fills exactly)
            const int64_t next = rb + (int64_t)rpw * R;
            if (next - buf_row >= kDotBuf || next >= r1) {
                const int64_t end = next < r1 ? next : r1;
                score_buffer<GRAD>(dots, (int)(end - buf_row), dsc.y, buf_row, margins, lane, loss_acc, ok_acc);
                buf_row = end;
            }
        }
        loss_acc = wave_sum(loss_acc);
        ok_acc = wave_sum(ok_acc);
        if (lane == 0) {
            tile_loss[item] = loss_acc;
            tile_ok[item] = ok_acc;
        }
    }
}

// CSR rows: one row per group of gl lanes (16, 32 or 64 by the partition's longest row), rows longer
// than the group looped over; col and val are streamed, w[col] gathered as f64 from HBM / L2. A row
// without non-zeros gives dot = 0.
template <typename S, int GRAD>
__global__ __launch_bounds__(kEvalBlock) void score_csr(const ChainDesc* __restrict__ descs,
                                                        const EvalPart* __restrict__ ep, int P,
                                                        int64_t n_items, const double* __restrict__ w,
                                                        double* __restrict__ tile_loss,
                                                        double* __restrict__ tile_ok,
                                                        double* __restrict__ margins) {
    __shared__ double dots_sh[kEvalWaves][kDotBuf];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t base = ep[0].tile0;
    for (int64_t item = (int64_t)blockIdx.x * kEvalWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kEvalWaves) {
        const int p = item_partition(ep, P, item);
        const ChainDesc dsc = descs[p];
        const int gl = ep[p].group;
        const int rpw = 64 / gl;
        const int g = lane / gl, j = lane & (gl - 1);
        const int64_t r0 = (item - (ep[p].tile0 - base)) * ep[p].tile_rows;
        const int64_t r1 = r0 + ep[p].tile_rows < dsc.n_rows ? r0 + ep[p].tile_rows : dsc.n_rows;
        const S* val = reinterpret_cast<const S*>(dsc.x);
        double* dots = dots_sh[wave];
        int64_t buf_row = r0;   // the partition row of dots[0]
        double loss_acc = 0.0, ok_acc = 0.0;
        for (int64_t rb = r0; rb < r1; rb += rpw) {
            const int64_t r = rb + g;
            const bool valid = r < r1;
            const int64_t rr = valid ? r : r0;
            const int64_t s = dsc.row_ptr[rr];
            const int64_t e = valid ? dsc.row_ptr[rr + 1] : s;
            double acc = 0.0;
            for (int64_t k = s + j; k < e; k += gl)
                acc = __builtin_fma((double)__builtin_nontemporal_load(as_global(val + k)),
                                    w[__builtin_nontemporal_load(as_global(dsc.col + k))], acc);
            const double dot = group_sum(acc, gl);
            if (valid && j == 0) dots[rr - buf_row] = dot;
            const int64_t next = rb + rpw;
            if (next - buf_row >= kDotBuf || next >= r1) {
                const int64_t end = next < r1 ? next : r1;
                score_buffer<GRAD>(dots, (int)(end - buf_row), dsc.y, buf_row, margins, lane, loss_acc, ok_acc);
                buf_row = end;
            }
        }
        loss_acc = wave_sum(loss_acc);
        ok_acc = wave_sum(ok_acc);
        if (lane == 0) {
            tile_loss[item] = loss_acc;
            tile_ok[item] = ok_acc;
        }
    }
}

// v[0] + v[1] + ... + v[n - 1], left to right, by one wave: 64 values per load (the next 64 in
// flight meanwhile), added in lane order -- one dependent v_add_f64 per value, the lanes read with
// constant indices.
__device__ __forceinline__ double ordered_sum(const double* v, int64_t n, int lane) {
    double s = 0.0;
    double x = lane < n ? v[lane] : 0.0;
    int64_t b = 0;
    for (; b + 64 <= n; b += 64) {
        const double nx = b + 64 + lane < n ? v[b + 64 + lane] : 0.0;
#pragma unroll
        for (int k = 0; k < 64; ++k) s += readlane_d(x, k);
        x = nx;
    }
    const int m = (int)(n - b);
    for (int k = 0; k < m; ++k) s += readlane_d(x, k);
    return s;
}
// The same sum of whole numbers (the tiles' correct predictions): exact in any order.
__device__ __forceinline__ double count_sum(const double* v, int64_t n, int lane) {
    double s = 0.0;
    for (int64_t i = lane; i < n; i += 64) s += v[i];
    return wave_sum(s);
}

// One workgroup: each wave adds the tiles of partitions wave, wave + 16, ... in tile order into
// part[2 p] = lossSum_p, part[2 p + 1] = nCorrect_p; then wave 0 adds the partitions in
// partition-index order: out3 = {lossSum, count, nCorrect}.
__global__ __launch_bounds__(kReduceBlock) void eval_reduce(const ChainDesc* __restrict__ descs,
                                                            const EvalPart* __restrict__ ep, int P,
                                                            const double* __restrict__ tile_loss,
                                                            const double* __restrict__ tile_ok,
                                                            double* part, double* __restrict__ part_out,
                                                            double* __restrict__ out3) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ long long rows_sh[kReduceBlock / 64];
    const int64_t base = P > 0 ? ep[0].tile0 : 0;
    for (int p = wave; p < P; p += kReduceBlock / 64) {
        const int64_t t0 = ep[p].tile0 - base, nt = ep[p + 1].tile0 - ep[p].tile0;
        const double s = ordered_sum(tile_loss + t0, nt, lane);
        const double c = count_sum(tile_ok + t0, nt, lane);
        if (lane == 0) {
            part[2 * p] = s;
            part[2 * p + 1] = c;
            if (part_out) {
                part_out[2 * p] = s;
                part_out[2 * p + 1] = c;
            }
        }
    }
    // count = the registered rows (integers: any order)
    long long rows = 0;
    for (int p = threadIdx.x; p < P; p += kReduceBlock) rows += descs[p].n_rows;
    for (int m = 32; m >= 1; m >>= 1) rows += __shfl_xor(rows, m, 64);
    if (lane == 0) rows_sh[wave] = rows;
    __threadfence();
    __syncthreads();
    if (wave != 0) return;
    // part holds 2 P doubles {loss, correct} interleaved: split the two sums by stride
    double s = 0.0, c = 0.0;
    for (int b = 0; b < P; b += 64) {
        const double xs = b + lane < P ? part[2 * (b + lane)] : 0.0;
        const double xc = b + lane < P ? part[2 * (b + lane) + 1] : 0.0;
        const int m = P - b < 64 ? P - b : 64;
        for (int k = 0; k < m; ++k) {
            s += readlane_d(xs, k);
            c += readlane_d(xc, k);
        }
    }
    if (lane == 0) {
        long long total = 0;
        for (int k = 0; k < kReduceBlock / 64; ++k) total += rows_sh[k];
        out3[0] = s;
        out3[1] = (double)total;
        out3[2] = c;
    }
}

template <typename S, int GRAD>
int launch_score_sg(const ChainDesc* descs, const EvalPart* ep, int P, int64_t n_items, int layout,
                    const double* w, int d, double* tile_loss, double* tile_ok, double* margins,
                    unsigned blocks, hipStream_t st) {
    if (layout == kCsr) {
        hipLaunchKernelGGL((score_csr<S, GRAD>), dim3(blocks), dim3(kEvalBlock), 0, st, descs, ep, P, n_items,
                           w, tile_loss, tile_ok, margins);
    } else if (d <= kEvalWLds) {
        const size_t lds = ((size_t)d * sizeof(double) + 15) & ~(size_t)15;
        hipLaunchKernelGGL((score_dense<S, GRAD, true>), dim3(blocks), dim3(kEvalBlock), lds, st, descs, ep, P,
                           n_items, w, d, tile_loss, tile_ok, margins);
    } else {
        hipLaunchKernelGGL((score_dense<S, GRAD, false>), dim3(blocks), dim3(kEvalBlock), 0, st, descs, ep, P,
                           n_items, w, d, tile_loss, tile_ok, margins);
    }
    return (int)hipGetLastError();
}

template <typename S>
int launch_score_s(int gradient, const ChainDesc* descs, const EvalPart* ep, int P, int64_t n_items,
                   int layout, const double* w, int d, double* tile_loss, double* tile_ok, double* margins,
                   unsigned blocks, hipStream_t st) {
    switch (gradient) {
        case G_LOGISTIC:
            return launch_score_sg<S, G_LOGISTIC>(descs, ep, P, n_items, layout, w, d, tile_loss, tile_ok,
                                                  margins, blocks, st);
        case G_LEAST_SQUARES:
            return launch_score_sg<S, G_LEAST_SQUARES>(descs, ep, P, n_items, layout, w, d, tile_loss, tile_ok,
                                                       margins, blocks, st);
        case G_HINGE:
            return launch_score_sg<S, G_HINGE>(descs, ep, P, n_items, layout, w, d, tile_loss, tile_ok,
                                               margins, blocks, st);
    }
    return -2;
}

}  // namespace

void eval_geometry(int layout, int64_t row_bytes, int64_t max_nnz, int32_t* tile_rows, int32_t* group) {
    if (layout == kCsr) {
        *group = max_nnz <= 16 ? 16 : max_nnz <= 32 ? 32 : 64;
        *tile_rows = 512;
        return;
    }
    int gl = 64;
    if (row_bytes < 1024) {
        gl = 1;
        while ((int64_t)gl * 16 < row_bytes) gl *= 2;
    }
    // ~252 KiB of rows a tile, between 16 and 1,024 rows: large enough that the tile partials are
    // nothing beside the rows (16 bytes a tile), small enough that a few partitions still give every
    // wave of the grid many tiles
    int64_t tr = ((int64_t)252 * 1024) / (row_bytes > 0 ? row_bytes : 1);
    tr = tr < 16 ? 16 : tr > 1024 ? 1024 : tr;
    *group = gl;
    *tile_rows = (int32_t)tr;
}

int launch_score(const ChainDesc* descs, const EvalPart* ep, int n_parts, int64_t n_items, int layout,
                 int storage, int gradient, const double* w, int d, double* tile_loss, double* tile_ok,
                 double* margins, int num_cus, hipStream_t st) {
    if (n_items <= 0) return 0;
    // a persistent grid: 8 workgroups of 4 waves a CU, fewer when there are fewer tiles than waves
    const int64_t want = (n_items + kEvalWaves - 1) / kEvalWaves;
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 8;
    const unsigned blocks = (unsigned)(want < cap ? want : cap);
    return storage == 1 ? launch_score_s<float>(gradient, descs, ep, n_parts, n_items, layout, w, d, tile_loss,
                                                tile_ok, margins, blocks, st)
                        : launch_score_s<double>(gradient, descs, ep, n_parts, n_items, layout, w, d, tile_loss,
                                                 tile_ok, margins, blocks, st);
}

int launch_eval_reduce(const ChainDesc* descs, const EvalPart* ep, int n_parts, const double* tile_loss,
                       const double* tile_ok, double* part, double* part_out, double* out3, hipStream_t st) {
    hipLaunchKernelGGL(eval_reduce, dim3(1), dim3(kReduceBlock), 0, st, descs, ep, n_parts, tile_loss, tile_ok,
                       part, part_out, out3);
    return (int)hipGetLastError();
}

}  // namespace psgd
