// psgd_colstats.hip -- column statistics over the registered partitions (psgd_column_stats) and
// the in-place column transform of the context's own rows (psgd_transform_columns): what MLlib
// 1.6.1's MultivariateOnlineSummarizer and StandardScalerModel.transform compute, in fp64 whatever
// the storage.
//
// No chain, as in psgd_eval.hip: the rows are cut into tiles numbered across the partitions in
// partition-index order (tile0[p] is partition p's first tile), taken by the waves of a persistent
// grid.
//
// Dense rows, bitwise reproducible: a work item is (tile, column chunk). Lanes lie across a row's
// 16-byte vectors, so a lane owns fixed columns and keeps their accumulators in registers over the
// tile's rows: s1 = sum(x - K), s2 = sum((x - K)^2) with K the column's value in the tile's first
// row (two additions and one fma an element, no division), the non-zero count, max and min. The
// tile's record is mean = K + s1 / m, M2 = s2 - s1^2 / m (K is one of the samples, so the
// cancellation is bounded by the tile's row count; a constant column gives s1 = s2 = 0 and mean = K,
// M2 = 0 exactly). stats_merge folds the records with Chan's formula in tile order -- first spans
// of consecutive tiles, then the spans in order: tile order is partition-index order. Every order
// is fixed by the registry's geometry: no floating-point atomics, the same bits from call to call
// and for any grid size.
//
// CSR rows, NOT bitwise reproducible in mean and m2: columns scatter over up to 2^22 features, so
// two streaming passes add into the output with fp64 vector atomics: pass 1 sum(x), the non-zero
// count (integer atomics), max and min (integer atomics on order-preserving keys, issued only when
// a plain read shows the value would move the extreme); pass 2 sum over the non-zeros of
// (x - mean)^2, to which (n - nnz) mean^2 is added for the absent entries. Sums of whole numbers
// (a column of 1.0) and of nothing are exact in any order. count, numNonzeros, max and min are
// exact and reproducible; mean and m2 may differ in their last bits from run to run.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include "psgd_device.h"

namespace psgd {
namespace {

constexpr int kStatBlock = 256;
constexpr int kStatWaves = kStatBlock / 64;
constexpr int kStatRows = 4;   // rows a lane keeps in flight
constexpr int kStatVecs = 2;   // 16-byte vectors of a row a lane owns: a chunk is 2 KiB of the row

// The tile's partition: the last p with tile0[p] <= tile (empty partitions share their first tile
// with the next one). Wave-uniform.
__device__ __forceinline__ int tile_partition(const int64_t* tile0, int P, int64_t tile) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile0[mid] <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename S>
__global__ __launch_bounds__(kStatBlock) void stats_dense(const ChainDesc* __restrict__ descs,
                                                          const int64_t* __restrict__ tile0, int P,
                                                          int64_t n_items, StatGeom gm,
                                                          double* __restrict__ rec, double* __restrict__ rec_m) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int U = kStatVecs, R = kStatRows;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gl = gm.group, rpw = 64 / gl;
    const int g = lane / gl, j = lane & (gl - 1);
    const int d = gm.d;
    for (int64_t item = (int64_t)blockIdx.x * kStatWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kStatWaves) {
        const int64_t tile = item / gm.n_chunks;
        const int chunk = (int)(item - tile * gm.n_chunks);
        const int p = tile_partition(tile0, P, tile);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        // the lane's vectors; one past the row's last reads vector 0 instead and is never written
        int v[U], vc[U];
        bool vok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v[u] = (chunk * U + u) * gl + j;
            vok[u] = v[u] < gm.nvec;
            vc[u] = vok[u] ? v[u] : 0;
        }
        double K[U][VEC], s1[U][VEC], s2[U][VEC];
        S mx[U][VEC], mn[U][VEC];
        int nz[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            S k0[VEC];
            unpack<S, S>(__builtin_nontemporal_load(as_global(reinterpret_cast<const V*>(X + r0 * dsc.ld) + vc[u])), k0);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                K[u][e] = (double)k0[e];
                s1[u][e] = 0.0;
                s2[u][e] = 0.0;
                mx[u][e] = k0[e];
                mn[u][e] = k0[e];
                nz[u][e] = 0;
            }
        }
        for (int64_t rb = r0; rb < r1; rb += (int64_t)rpw * R) {
            V xv[R][U];
            bool valid[R];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const int64_t r = rb + (int64_t)q * rpw + g;
                valid[q] = r < r1;
                // (a lane group past the tile's end re-reads the first row: x - K = 0 there)
                const V* row = reinterpret_cast<const V*>(X + (valid[q] ? r : r0) * dsc.ld);
#pragma unroll
                for (int u = 0; u < U; ++u) xv[q][u] = __builtin_nontemporal_load(as_global(row + vc[u]));
            }
#pragma unroll
            for (int q = 0; q < R; ++q) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    S x[VEC];
                    unpack<S, S>(xv[q][u], x);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const double t = (double)x[e] - K[u][e];
                        s1[u][e] += t;
                        s2[u][e] = __builtin_fma(t, t, s2[u][e]);
                        nz[u][e] += (valid[q] && x[e] != S(0)) ? 1 : 0;
                        mx[u][e] = x[e] > mx[u][e] ? x[e] : mx[u][e];
                        mn[u][e] = x[e] < mn[u][e] ? x[e] : mn[u][e];
                    }
                }
            }
        }
        // narrow rows: the wave's 64 / gl lane groups hold different rows of the same columns, all
        // shifted by the same K: their sums add, in an order the geometry fixes
        for (int m = gl; m < 64; m <<= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    s1[u][e] += __shfl_xor(s1[u][e], m, 64);
                    s2[u][e] += __shfl_xor(s2[u][e], m, 64);
                    nz[u][e] += __shfl_xor(nz[u][e], m, 64);
                    const S ox = __shfl_xor(mx[u][e], m, 64), on = __shfl_xor(mn[u][e], m, 64);
                    mx[u][e] = ox > mx[u][e] ? ox : mx[u][e];
                    mn[u][e] = on < mn[u][e] ? on : mn[u][e];
                }
            }
        }
        const double m = (double)(r1 - r0);
        if (g == 0) {
            double* out = rec + tile * 5 * (int64_t)d;
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int c = v[u] * VEC + e;
                    if (vok[u] && c < d) {
                        const double a = s1[u][e] / m;
                        const double m2 = __builtin_fma(-a, s1[u][e], s2[u][e]);
                        out[c] = K[u][e] + a;
                        out[(int64_t)d + c] = m2 > 0.0 ? m2 : 0.0;
                        out[2 * (int64_t)d + c] = (double)nz[u][e];
                        out[3 * (int64_t)d + c] = (double)mx[u][e];
                        out[4 * (int64_t)d + c] = (double)mn[u][e];
                    }
                }
            }
        }
        if (chunk == 0 && lane == 0) rec_m[tile] = m;
    }
}

// Records [T][5][d] = {mean, M2, numNonzeros, max, min} of src_m[t] rows each: thread (column,
// span) merges records [span * s, span * (s + 1)) in order with Chan's formula into dst[s], and
// their rows into dst_m[s]. Empty operands are skipped.
__global__ __launch_bounds__(kStatBlock) void stats_merge(const double* __restrict__ src,
                                                          const double* __restrict__ src_m, int64_t T,
                                                          int64_t span, double* __restrict__ dst,
                                                          double* __restrict__ dst_m, int d) {
    const int c = blockIdx.x * kStatBlock + threadIdx.x;
    const int64_t s = blockIdx.y;
    if (c >= d) return;
    const int64_t t0 = s * span, t1 = t0 + span < T ? t0 + span : T;
    double na = 0.0, mean = 0.0, M2 = 0.0, nz = 0.0, mx = 0.0, mn = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const double nb = src_m[t];
        if (nb == 0.0) continue;
        const double* r = src + t * 5 * (int64_t)d + c;
        const double mean_b = r[0], M2_b = r[d], nz_b = r[2 * (int64_t)d], mx_b = r[3 * (int64_t)d],
                     mn_b = r[4 * (int64_t)d];
        if (na == 0.0) {
            na = nb; mean = mean_b; M2 = M2_b; nz = nz_b; mx = mx_b; mn = mn_b;
            continue;
        }
        const double n = na + nb;
        const double delta = mean_b - mean;
        mean = mean + delta * (nb / n);
        M2 = M2 + M2_b + delta * delta * (na * nb / n);
        nz += nz_b;
        mx = mx_b > mx ? mx_b : mx;
        mn = mn_b < mn ? mn_b : mn;
        na = n;
    }
    double* o = dst + s * 5 * (int64_t)d + c;
    o[0] = mean;
    o[d] = M2;
    o[2 * (int64_t)d] = nz;
    o[3 * (int64_t)d] = mx;
    o[4 * (int64_t)d] = mn;
    if (c == 0) dst_m[s] = na;
}

// ---- CSR ----
// Order-preserving key of a double: a < b <=> key(a) < key(b) as unsigned integers.
__device__ __forceinline__ unsigned long long order_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// out = {count, mean[d], m2[d], numNonzeros[d], max[d], min[d]} doubles; during the passes the
// mean slot holds sum(x), the numNonzeros slot a 64-bit count, the max / min slots keys.
__global__ __launch_bounds__(kStatBlock) void csr_stats_init(double* __restrict__ out, int d, double n) {
    const int64_t c = (int64_t)blockIdx.x * kStatBlock + threadIdx.x;
    if (c == 0) out[0] = n;
    if (c >= d) return;
    unsigned long long* u = reinterpret_cast<unsigned long long*>(out + 1);
    out[1 + c] = 0.0;
    out[1 + d + c] = 0.0;
    u[2 * (int64_t)d + c] = 0ull;
    u[3 * (int64_t)d + c] = 0ull;      // below every key
    u[4 * (int64_t)d + c] = ~0ull;     // above every key
}

// PASS 1: sum, count, max, min of the stored non-zeros; PASS 2: sum of (x - mean)^2 over them.
// A tile's non-zeros are one contiguous range of col / val: 64 consecutive ones a wave instruction.
template <typename S, int PASS>
__global__ __launch_bounds__(kStatBlock) void stats_csr(const ChainDesc* __restrict__ descs,
                                                        const int64_t* __restrict__ tile0, int P,
                                                        int64_t n_items, StatGeom gm, double* out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t d = gm.d;
    double* sum = out + 1;              // pass 2: the means
    double* m2 = out + 1 + d;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(out + 1) + 2 * d;
    unsigned long long* kmax = cnt + d;
    unsigned long long* kmin = kmax + d;
    for (int64_t item = (int64_t)blockIdx.x * kStatWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kStatWaves) {
        const int p = tile_partition(tile0, P, item);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (item - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        const S* val = reinterpret_cast<const S*>(dsc.x);
        const int64_t k1 = dsc.row_ptr[r1];
        for (int64_t k = dsc.row_ptr[r0] + lane; k < k1; k += 64) {
            const double x = (double)__builtin_nontemporal_load(as_global(val + k));
            const int c = __builtin_nontemporal_load(as_global(dsc.col + k));
            if (x == 0.0) continue;   // an explicitly stored 0.0 is an absent entry
            if constexpr (PASS == 1) {
                unsafeAtomicAdd(sum + c, x);
                atomicAdd(cnt + c, 1ull);
                // the extremes only move outwards: a stale read can only cause a needless atomic
                const unsigned long long key = order_key(x);
                if (key > __hip_atomic_load(kmax + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(kmax + c, key);
                if (key < __hip_atomic_load(kmin + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(kmin + c, key);
            } else {
                const double t = x - sum[c];
                unsafeAtomicAdd(m2 + c, t * t);
            }
        }
    }
}

__global__ __launch_bounds__(kStatBlock) void csr_stats_mean(double* __restrict__ out, int d, double n) {
    const int64_t c = (int64_t)blockIdx.x * kStatBlock + threadIdx.x;
    if (c >= d) return;
    out[1 + c] = n > 0.0 ? out[1 + c] / n : 0.0;
}

__global__ __launch_bounds__(kStatBlock) void csr_stats_final(double* __restrict__ out, int d, double n) {
    const int64_t c = (int64_t)blockIdx.x * kStatBlock + threadIdx.x;
    if (c >= d) return;
    unsigned long long* u = reinterpret_cast<unsigned long long*>(out + 1);
    const unsigned long long cnt = u[2 * (int64_t)d + c];
    const double nnz = (double)cnt, mean = out[1 + c];
    double mx = cnt ? key_value(u[3 * (int64_t)d + c]) : 0.0;
    double mn = cnt ? key_value(u[4 * (int64_t)d + c]) : 0.0;
    if (nnz < n) {   // the absent entries take part with 0.0
        mx = mx > 0.0 ? mx : 0.0;
        mn = mn < 0.0 ? mn : 0.0;
    }
    out[1 + d + c] = out[1 + d + c] + (n - nnz) * (mean * mean);
    out[1 + 2 * (int64_t)d + c] = nnz;
    out[1 + 3 * (int64_t)d + c] = mx;
    out[1 + 4 * (int64_t)d + c] = mn;
}

// ---- Transform ----
// x' = round_to_storage(((double)x - shift[c]) * factor[c]) over columns < d of the tile's rows, in
// place; the pad columns [d, ld) keep their bits (zeros: the chains rely on them).
template <typename S, bool SHIFT>
__global__ __launch_bounds__(kStatBlock) void transform_dense(const ChainDesc* __restrict__ descs,
                                                              const int64_t* __restrict__ tile0, int P,
                                                              int64_t n_items, StatGeom gm,
                                                              const double* __restrict__ shift,
                                                              const double* __restrict__ factor) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int R = kStatRows;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gl = gm.group, rpw = 64 / gl;
    const int g = lane / gl, j = lane & (gl - 1);
    const int d = gm.d;
    for (int64_t item = (int64_t)blockIdx.x * kStatWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kStatWaves) {
        const int p = tile_partition(tile0, P, item);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (item - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        S* X = reinterpret_cast<S*>(const_cast<void*>(dsc.x));
        for (int64_t rb = r0; rb < r1; rb += (int64_t)rpw * R) {
            for (int vv = j; vv < gm.nvec; vv += gl) {
                double f[VEC], sh[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int c = vv * VEC + e;
                    f[e] = c < d ? factor[c] : 1.0;
                    sh[e] = (SHIFT && c < d) ? shift[c] : 0.0;
                }
                V xv[R];
                V* at[R];
                bool valid[R];
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    const int64_t r = rb + (int64_t)q * rpw + g;
                    valid[q] = r < r1;
                    at[q] = reinterpret_cast<V*>(X + (valid[q] ? r : r0) * dsc.ld) + vv;
                    xv[q] = __builtin_nontemporal_load(as_global(at[q]));
                }
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    if (!valid[q]) continue;
                    V o = xv[q];
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        if (vv * VEC + e < d) {
                            double t = (double)xv[q][e];
                            if constexpr (SHIFT) t = t - sh[e];
                            o[e] = (S)(t * f[e]);
                        }
                    }
                    *at[q] = o;
                }
            }
        }
    }
}

// val[k] = round_to_storage((double)val[k] * factor[col[k]]) over the tile's non-zeros.
template <typename S>
__global__ __launch_bounds__(kStatBlock) void transform_csr(const ChainDesc* __restrict__ descs,
                                                            const int64_t* __restrict__ tile0, int P,
                                                            int64_t n_items, StatGeom gm,
                                                            const double* __restrict__ factor) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int64_t item = (int64_t)blockIdx.x * kStatWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kStatWaves) {
        const int p = tile_partition(tile0, P, item);
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (item - tile0[p]) * gm.tile_rows;
        const int64_t r1 = r0 + gm.tile_rows < dsc.n_rows ? r0 + gm.tile_rows : dsc.n_rows;
        S* val = reinterpret_cast<S*>(const_cast<void*>(dsc.x));
        const int64_t k1 = dsc.row_ptr[r1];
        for (int64_t k = dsc.row_ptr[r0] + lane; k < k1; k += 64) {
            const double x = (double)__builtin_nontemporal_load(as_global(val + k));
            const int c = __builtin_nontemporal_load(as_global(dsc.col + k));
            val[k] = (S)(x * factor[c]);
        }
    }
}

// A persistent grid of at most 8 workgroups a CU in which every wave takes the same number of
// items (to within one): with fewer items than two rounds of the full grid, a full grid would
// leave most waves idle during the second round.
unsigned balanced_blocks(int64_t n_items, int num_cus) {
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 8 * kStatWaves;
    const int64_t rounds = (n_items + cap - 1) / cap;
    const int64_t waves = (n_items + rounds - 1) / rounds;
    return (unsigned)((waves + kStatWaves - 1) / kStatWaves);
}

unsigned column_blocks(int d) { return (unsigned)((d + kStatBlock - 1) / kStatBlock); }

}  // namespace

StatGeom stats_geometry(int layout, int d, int storage) {
    StatGeom gm{};
    gm.d = d;
    if (layout == kCsr) {
        gm.group = 64;
        gm.nvec = 0;
        gm.n_chunks = 1;
        gm.tile_rows = 512;
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
    gm.n_chunks = (gm.nvec + gl * kStatVecs - 1) / (gl * kStatVecs);
    // a tile's record is 40 bytes a column: a hundredth of 1,024 f32 or 512 f64 rows
    gm.tile_rows = storage == 1 ? 1024 : 512;
    return gm;
}

int64_t stats_merge_span(int64_t n_tiles) {
    int64_t s = 32;
    while (s * s < n_tiles) ++s;
    return s;
}

int launch_stats_dense(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                       const StatGeom& gm, int storage, double* rec, double* rec_m, double* rec2, double* rec2_m,
                       double* out, int num_cus, hipStream_t st) {
    if (n_tiles <= 0) return (int)hipMemsetAsync(out, 0, (1 + 5 * (size_t)gm.d) * sizeof(double), st);
    const int64_t n_items = n_tiles * gm.n_chunks;
    const unsigned blocks = balanced_blocks(n_items, num_cus);
    if (storage == 1)
        hipLaunchKernelGGL(stats_dense<float>, dim3(blocks), dim3(kStatBlock), 0, st, descs, tile0, n_parts, n_items,
                           gm, rec, rec_m);
    else
        hipLaunchKernelGGL(stats_dense<double>, dim3(blocks), dim3(kStatBlock), 0, st, descs, tile0, n_parts, n_items,
                           gm, rec, rec_m);
    int e = (int)hipGetLastError();
    if (e) return e;
    const int64_t span = stats_merge_span(n_tiles);
    const int64_t n_spans = (n_tiles + span - 1) / span;
    hipLaunchKernelGGL(stats_merge, dim3(column_blocks(gm.d), (unsigned)n_spans), dim3(kStatBlock), 0, st, rec, rec_m,
                       n_tiles, span, rec2, rec2_m, gm.d);
    e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(stats_merge, dim3(column_blocks(gm.d), 1), dim3(kStatBlock), 0, st, rec2, rec2_m, n_spans,
                       n_spans, out + 1, out, gm.d);
    return (int)hipGetLastError();
}

int launch_stats_csr(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles, int64_t n_rows,
                     const StatGeom& gm, int storage, double* out, int num_cus, hipStream_t st) {
    const double n = (double)n_rows;
    const unsigned cb = column_blocks(gm.d);
    hipLaunchKernelGGL(csr_stats_init, dim3(cb), dim3(kStatBlock), 0, st, out, gm.d, n);
    int e = (int)hipGetLastError();
    if (e) return e;
    const unsigned blocks = n_tiles > 0 ? balanced_blocks(n_tiles, num_cus) : 0;
    if (blocks) {
        if (storage == 1)
            hipLaunchKernelGGL((stats_csr<float, 1>), dim3(blocks), dim3(kStatBlock), 0, st, descs, tile0, n_parts,
                               n_tiles, gm, out);
        else
            hipLaunchKernelGGL((stats_csr<double, 1>), dim3(blocks), dim3(kStatBlock), 0, st, descs, tile0, n_parts,
                               n_tiles, gm, out);
        if ((e = (int)hipGetLastError())) return e;
    }
    hipLaunchKernelGGL(csr_stats_mean, dim3(cb), dim3(kStatBlock), 0, st, out, gm.d, n);
    if ((e = (int)hipGetLastError())) return e;
    if (blocks) {
        if (storage == 1)
            hipLaunchKernelGGL((stats_csr<float, 2>), dim3(blocks), dim3(kStatBlock), 0, st, descs, tile0, n_parts,
                               n_tiles, gm, out);
        else
            hipLaunchKernelGGL((stats_csr<double, 2>), dim3(blocks), dim3(kStatBlock), 0, st, descs, tile0, n_parts,
                               n_tiles, gm, out);
        if ((e = (int)hipGetLastError())) return e;
    }
    hipLaunchKernelGGL(csr_stats_final, dim3(cb), dim3(kStatBlock), 0, st, out, gm.d, n);
    return (int)hipGetLastError();
}

int launch_transform(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles, int layout,
                     const StatGeom& gm, int storage, const double* shift, const double* factor, int num_cus,
                     hipStream_t st) {
    if (n_tiles <= 0) return 0;
    const unsigned blocks = balanced_blocks(n_tiles, num_cus);
    const dim3 gr(blocks), bl(kStatBlock);
    if (layout == kCsr) {
        if (storage == 1)
            hipLaunchKernelGGL(transform_csr<float>, gr, bl, 0, st, descs, tile0, n_parts, n_tiles, gm, factor);
        else
            hipLaunchKernelGGL(transform_csr<double>, gr, bl, 0, st, descs, tile0, n_parts, n_tiles, gm, factor);
    } else if (storage == 1) {
        if (shift)
            hipLaunchKernelGGL((transform_dense<float, true>), gr, bl, 0, st, descs, tile0, n_parts, n_tiles, gm, shift, factor);
        else
            hipLaunchKernelGGL((transform_dense<float, false>), gr, bl, 0, st, descs, tile0, n_parts, n_tiles, gm, shift, factor);
    } else {
        if (shift)
            hipLaunchKernelGGL((transform_dense<double, true>), gr, bl, 0, st, descs, tile0, n_parts, n_tiles, gm, shift, factor);
        else
            hipLaunchKernelGGL((transform_dense<double, false>), gr, bl, 0, st, descs, tile0, n_parts, n_tiles, gm, shift, factor);
    }
    return (int)hipGetLastError();
}

}  // namespace psgd
