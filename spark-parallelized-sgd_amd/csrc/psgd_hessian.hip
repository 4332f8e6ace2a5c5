// psgd_hessian.hip -- the rows' curvature at fixed weights (psgd_row_curvature): for every registered
// row h_i = d^2 loss / d(x_i . w)^2, one double per row in local row order (the partitions in
// partition-index order, a partition's rows in iterator order; row0[p] is partition p's first row).
// With it as the row weight of the weighted Gramian (psgd_gram.hip), M_h[:d, :d] is the Hessian of the
// loss sum.
//
//   Logistic:      z = x . w in fp64 (fma along the features), e = exp(-|z|), h = e / ((1 + e)(1 + e)):
//                  sigma(z) (1 - sigma(z)) written so that it is exactly 0.25 at z = 0, exactly 0.0 once
//                  e underflows, and never NaN for a finite z
//   LeastSquares:  h = 1.0 (the rows are not read)
//
// One launch over all partitions. The row walk is the scoring pass's (psgd_eval.hip: the same tiling,
// EvalPart, the same lane groups across a row's 16-byte vectors or a CSR row's entries, the dots
// parked in a wave's own LDS buffer so that every lane carries the exp of a row); every row is
// independent and written once: the same bits from call to call.
#include "psgd_device.h"
#include "psgd_eval.h"

namespace psgd {
namespace {

constexpr int kCurvBlock = 256;
constexpr int kCurvWaves = kCurvBlock / 64;
constexpr int kCurvRows = 4;      // dense: rows a lane group keeps in flight
constexpr int kCurvWLds = 4096;   // dense: weights of up to this many features live in LDS
constexpr int kCurvBuf = 256;     // dots a wave parks before it takes their curvature

__device__ __forceinline__ double logistic_curvature(double z) {
    const double e = exp(-fabs(z));
    const double q = 1.0 + e;
    return e / (q * q);
}

// buf[0 .. n) are the dots of local rows first .. first + n: row i of the buffer in lane i % 64.
__device__ __forceinline__ void curvature_buffer(const double* buf, int n, double* __restrict__ out, int64_t first,
                                                 int lane) {
    wave_lds_sync();
    for (int i = lane; i < n; i += 64) out[first + i] = logistic_curvature(buf[i]);
    wave_lds_sync();
}

template <typename S, bool WLDS>
__global__ __launch_bounds__(kCurvBlock) void curvature_dense(const ChainDesc* __restrict__ descs,
                                                              const EvalPart* __restrict__ ep,
                                                              const int64_t* __restrict__ row0, int P,
                                                              int64_t n_items, const double* __restrict__ w, int d,
                                                              double* __restrict__ out) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int R = kCurvRows;
    extern __shared__ __attribute__((aligned(16))) double w_lds[];
    __shared__ double dots_sh[kCurvWaves][kCurvBuf];
    if constexpr (WLDS) {
        for (int i = threadIdx.x; i < d; i += kCurvBlock) w_lds[i] = w[i];
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
    for (int64_t item = (int64_t)blockIdx.x * kCurvWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kCurvWaves) {
        const int p = item_partition(ep, P, item);
        const ChainDesc dsc = descs[p];
        const int gl = ep[p].group;
        const int rpw = 64 / gl;
        const int g = lane / gl, j = lane & (gl - 1);
        const int64_t r0 = (item - (ep[p].tile0 - base)) * ep[p].tile_rows;
        const int64_t r1 = r0 + ep[p].tile_rows < dsc.n_rows ? r0 + ep[p].tile_rows : dsc.n_rows;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        double* dots = dots_sh[wave];
        const int64_t first = row0[p];
        int64_t buf_row = r0;   // the partition row of dots[0]
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
                // the partial vector lies inside the row's pitch (ld * sizeof(S) is a multiple of 16):
                // its elements past d (pad columns, NaN for all the pass knows) are not used
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
            // (rpw * R divides kCurvBuf: the buffer fills exactly)
            const int64_t next = rb + (int64_t)rpw * R;
            if (next - buf_row >= kCurvBuf || next >= r1) {
                const int64_t end = next < r1 ? next : r1;
                curvature_buffer(dots, (int)(end - buf_row), out, first + buf_row, lane);
                buf_row = end;
            }
        }
    }
}

template <typename S>
__global__ __launch_bounds__(kCurvBlock) void curvature_csr(const ChainDesc* __restrict__ descs,
                                                            const EvalPart* __restrict__ ep,
                                                            const int64_t* __restrict__ row0, int P,
                                                            int64_t n_items, const double* __restrict__ w,
                                                            double* __restrict__ out) {
    __shared__ double dots_sh[kCurvWaves][kCurvBuf];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t base = ep[0].tile0;
    for (int64_t item = (int64_t)blockIdx.x * kCurvWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kCurvWaves) {
        const int p = item_partition(ep, P, item);
        const ChainDesc dsc = descs[p];
        const int gl = ep[p].group;
        const int rpw = 64 / gl;
        const int g = lane / gl, j = lane & (gl - 1);
        const int64_t r0 = (item - (ep[p].tile0 - base)) * ep[p].tile_rows;
        const int64_t r1 = r0 + ep[p].tile_rows < dsc.n_rows ? r0 + ep[p].tile_rows : dsc.n_rows;
        const S* val = reinterpret_cast<const S*>(dsc.x);
        double* dots = dots_sh[wave];
        const int64_t first = row0[p];
        int64_t buf_row = r0;   // the partition row of dots[0]
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
            if (next - buf_row >= kCurvBuf || next >= r1) {
                const int64_t end = next < r1 ? next : r1;
                curvature_buffer(dots, (int)(end - buf_row), out, first + buf_row, lane);
                buf_row = end;
            }
        }
    }
}

// LeastSquares: out[0 .. n) = 1.0.
__global__ __launch_bounds__(kCurvBlock) void curvature_ones(double* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kCurvBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCurvBlock)
        out[i] = 1.0;
}

template <typename S>
int launch_curvature_s(const ChainDesc* descs, const EvalPart* ep, const int64_t* row0, int P, int64_t n_items,
                       int layout, const double* w, int d, double* out, unsigned blocks, hipStream_t st) {
    if (layout == kCsr) {
        hipLaunchKernelGGL(curvature_csr<S>, dim3(blocks), dim3(kCurvBlock), 0, st, descs, ep, row0, P, n_items, w,
                           out);
    } else if (d <= kCurvWLds) {
        const size_t lds = ((size_t)d * sizeof(double) + 15) & ~(size_t)15;
        hipLaunchKernelGGL((curvature_dense<S, true>), dim3(blocks), dim3(kCurvBlock), lds, st, descs, ep, row0, P,
                           n_items, w, d, out);
    } else {
        hipLaunchKernelGGL((curvature_dense<S, false>), dim3(blocks), dim3(kCurvBlock), 0, st, descs, ep, row0, P,
                           n_items, w, d, out);
    }
    return (int)hipGetLastError();
}

}  // namespace

int launch_row_curvature(const ChainDesc* descs, const EvalPart* ep, const int64_t* row0, int n_parts,
                         int64_t n_items, int64_t n_rows, int layout, int storage, int gradient, const double* w,
                         int d, double* out, int num_cus, hipStream_t st) {
    if (n_items <= 0 || n_rows <= 0) return 0;
    const int64_t cus = num_cus > 0 ? num_cus : 256;
    if (gradient == G_LEAST_SQUARES) {
        const int64_t want = (n_rows + kCurvBlock - 1) / kCurvBlock;
        const unsigned blocks = (unsigned)(want < cus * 8 ? want : cus * 8);
        hipLaunchKernelGGL(curvature_ones, dim3(blocks), dim3(kCurvBlock), 0, st, out, n_rows);
        return (int)hipGetLastError();
    }
    if (gradient != G_LOGISTIC) return (int)hipErrorInvalidValue;
    // a persistent grid, as the scoring pass's: 8 workgroups of 4 waves a CU, fewer when there are
    // fewer tiles than waves
    const int64_t want = (n_items + kCurvWaves - 1) / kCurvWaves;
    const unsigned blocks = (unsigned)(want < cus * 8 ? want : cus * 8);
    return storage == 1
               ? launch_curvature_s<float>(descs, ep, row0, n_parts, n_items, layout, w, d, out, blocks, st)
               : launch_curvature_s<double>(descs, ep, row0, n_parts, n_items, layout, w, d, out, blocks, st);
}

}  // namespace psgd
