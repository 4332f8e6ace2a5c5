// psgd_datasplit.hip -- the row compaction behind randomSplit / kFold (psgd_gather_dense_device,
// psgd_gather_csr_device): the rows a cell sampler kept (cell_select, psgd_kernels.hip) copied out
// of the registered partitions into buffers of the caller's, in order, bit for bit.
//
// No chain, as in psgd_colstats.hip: a partition's kept rows are cut into tiles numbered across
// the partitions in partition-index order (SplitPart::tile0), so one launch serves every partition
// of a split however many there are. The kernels only move bits: no floating-point arithmetic, no
// atomics, plain vector loads and stores.
//
// Dense rows are a bandwidth kernel: lanes lie across a row's 16-byte vectors (a power-of-two
// group, 64 / group rows a wave instruction), a wave keeps kGatherRows x kGatherVecs vectors in
// flight, the index list is increasing so the reads only move forward; rows are read at the source
// pitch and written at the output pitch, the pad columns [d, ld_out) as zeros whatever the source
// holds there. Loads and stores are non-temporal: every byte is touched once.
//
// CSR rows take three passes over tiles of kCsrTile kept rows, a workgroup a tile: the tiles'
// length sums; their exclusive scan per partition (which also closes row_ptr with the total); then
// each tile scans its rows' lengths from its base, writes row_ptr and copies the col / val segments
// with a group of lanes a row (16, 32 or 64 by the longest registered row, as the batch gradient
// does). Rows without non-zeros copy nothing; rows longer than the group loop.
#include "psgd_device.h"

namespace psgd {
namespace {

constexpr int kGatherBlock = 256;
constexpr int kGatherWaves = kGatherBlock / 64;
constexpr int kGatherRows = 4;   // rows a lane group keeps in flight
constexpr int kGatherVecs = 2;   // 16-byte vectors of each of those rows
constexpr int kCsrTile = 256;    // kept rows a workgroup takes: one a thread

// The tile's partition: the last p with tab[p].tile0 <= tile (partitions without kept rows share
// their first tile with the next one). Uniform over the wave / workgroup.
__device__ __forceinline__ int split_partition(const SplitPart* tab, int P, int64_t tile) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename S>
__global__ __launch_bounds__(kGatherBlock) void gather_dense(const ChainDesc* __restrict__ descs,
                                                             const SplitPart* __restrict__ tab, int P,
                                                             int64_t n_items, int tile_rows, int d, int gl,
                                                             int nvec_out, int64_t ld_out) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int R = kGatherRows, U = kGatherVecs;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int rpw = 64 / gl;
    const int g = lane / gl, j = lane & (gl - 1);
    const int64_t step = (int64_t)rpw * R;
    for (int64_t item = (int64_t)blockIdx.x * kGatherWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kGatherWaves) {
        const int p = split_partition(tab, P, item);
        const SplitPart sp = tab[p];
        const ChainDesc dsc = descs[p];
        const int64_t k0 = (item - sp.tile0) * tile_rows;
        const int64_t k1 = k0 + tile_rows < sp.m ? k0 + tile_rows : sp.m;
        if (k0 >= k1) continue;
        const int32_t* __restrict__ rows = sp.rows;
        for (int64_t k = k0 + lane; k < k1; k += 64) sp.y[k] = dsc.y[rows[k]];
        const S* X = reinterpret_cast<const S*>(dsc.x);
        S* O = reinterpret_cast<S*>(sp.x);
        const int nvec_src = (int)(dsc.ld / VEC);
        // the indices of the next group of rows are fetched while this one is copied
        // (out-of-range slots read the tile's last row and store nothing)
        int64_t nxt[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int64_t k = k0 + (int64_t)q * rpw + g;
            nxt[q] = rows[k < k1 ? k : k1 - 1];
        }
        for (int64_t kb = k0; kb < k1; kb += step) {
            int64_t src[R];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                src[q] = nxt[q];
                const int64_t k = kb + step + (int64_t)q * rpw + g;
                nxt[q] = rows[k < k1 ? k : k1 - 1];
            }
            for (int v0 = j; v0 < nvec_out; v0 += gl * U) {
                V xv[U][R];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int vv = v0 + u * gl;
#pragma unroll
                    for (int q = 0; q < R; ++q) {
                        if (vv < nvec_src && vv < nvec_out)
                            xv[u][q] = __builtin_nontemporal_load(
                                as_global(reinterpret_cast<const V*>(X + src[q] * dsc.ld) + vv));
                        else
                            xv[u][q] = V(0);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int vv = v0 + u * gl;
                    if (vv >= nvec_out) continue;
#pragma unroll
                    for (int q = 0; q < R; ++q) {
                        const int64_t k = kb + (int64_t)q * rpw + g;
                        if (k >= k1) continue;
                        V o = xv[u][q];
                        if ((vv + 1) * VEC > d) {
#pragma unroll
                            for (int e = 0; e < VEC; ++e)
                                if (vv * VEC + e >= d) o[e] = S(0);
                        }
                        __builtin_nontemporal_store(o, reinterpret_cast<V*>(O + k * ld_out) + vv);
                    }
                }
            }
        }
    }
}

// Exclusive scan of v over the workgroup's kGatherBlock threads; *total gets the sum.
__device__ __forceinline__ int64_t block_scan(int64_t v, int64_t* sh, int64_t* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < kGatherBlock; off <<= 1) {
        const int64_t t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const int64_t incl = sh[tid];
    *total = sh[kGatherBlock - 1];
    __syncthreads();
    return incl - v;
}

// Pass 1: tile_sum[tile] = the non-zeros of the tile's kept rows.
__global__ __launch_bounds__(kGatherBlock) void csr_tile_sums(const ChainDesc* __restrict__ descs,
                                                              const SplitPart* __restrict__ tab, int P,
                                                              int64_t n_tiles, int64_t* __restrict__ tile_sum) {
    __shared__ int64_t sh[kGatherBlock];
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int p = split_partition(tab, P, tile);
        const SplitPart sp = tab[p];
        const int64_t* rp = descs[p].row_ptr;
        const int64_t k = (tile - sp.tile0) * kCsrTile + threadIdx.x;
        int64_t len = 0;
        if (k < sp.m) {
            const int64_t r = sp.rows[k];
            len = rp[r + 1] - rp[r];
        }
        int64_t total;
        block_scan(len, sh, &total);
        if (threadIdx.x == 0) tile_sum[tile] = total;
    }
}

// Pass 2, a workgroup a partition: its tiles' sums become their exclusive scan (each tile's first
// output entry), and row_ptr[m] the partition's total -- row_ptr[0] = 0 of a partition that kept nothing.
__global__ __launch_bounds__(kGatherBlock) void csr_tile_bases(const SplitPart* __restrict__ tab,
                                                               int64_t* __restrict__ tile_sum) {
    __shared__ int64_t sh[kGatherBlock];
    const int p = blockIdx.x;
    const SplitPart sp = tab[p];
    const int64_t t0 = sp.tile0, t1 = tab[p + 1].tile0;
    int64_t base = 0;
    for (int64_t tb = t0; tb < t1; tb += kGatherBlock) {
        const int64_t t = tb + threadIdx.x;
        const int64_t v = t < t1 ? tile_sum[t] : 0;
        int64_t total;
        const int64_t ex = block_scan(v, sh, &total);
        if (t < t1) tile_sum[t] = base + ex;
        base += total;
    }
    if (threadIdx.x == 0) sp.row_ptr[sp.m] = base;
}

// Pass 3: row_ptr, labels and the col / val segments of the tile's kept rows.
template <typename S>
__global__ __launch_bounds__(kGatherBlock) void gather_csr(const ChainDesc* __restrict__ descs,
                                                           const SplitPart* __restrict__ tab, int P,
                                                           int64_t n_tiles, int gl,
                                                           const int64_t* __restrict__ tile_base) {
    __shared__ int64_t sh[kGatherBlock];
    __shared__ int64_t s_src[kCsrTile];
    __shared__ int64_t s_dst[kCsrTile + 1];
    const int tid = threadIdx.x;
    const int g = tid / gl, j = tid & (gl - 1), groups = kGatherBlock / gl;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int p = split_partition(tab, P, tile);
        const SplitPart sp = tab[p];
        const ChainDesc dsc = descs[p];
        const int64_t k0 = (tile - sp.tile0) * kCsrTile;
        const int nk = (int)(sp.m - k0 < kCsrTile ? sp.m - k0 : kCsrTile);
        int64_t len = 0, s0 = 0, r = 0;
        if (tid < nk) {
            r = sp.rows[k0 + tid];
            s0 = dsc.row_ptr[r];
            len = dsc.row_ptr[r + 1] - s0;
        }
        int64_t total;
        const int64_t o0 = tile_base[tile] + block_scan(len, sh, &total);
        s_src[tid] = s0;
        s_dst[tid] = o0;
        if (tid == kGatherBlock - 1) s_dst[kCsrTile] = o0 + len;
        if (tid < nk) {
            sp.row_ptr[k0 + tid] = o0;
            sp.y[k0 + tid] = dsc.y[r];
        }
        __syncthreads();
        const S* val = reinterpret_cast<const S*>(dsc.x);
        S* val_out = reinterpret_cast<S*>(sp.x);
        for (int q = g; q < nk; q += groups) {
            const int64_t s = s_src[q], o = s_dst[q];
            const int64_t n = s_dst[q + 1] - o;
            for (int64_t e = j; e < n; e += gl) {
                const int32_t c = __builtin_nontemporal_load(as_global(dsc.col + s + e));
                const S x = __builtin_nontemporal_load(as_global(val + s + e));
                __builtin_nontemporal_store(c, sp.col + o + e);
                __builtin_nontemporal_store(x, val_out + o + e);
            }
        }
        __syncthreads();   // s_src / s_dst are rewritten by the next tile
    }
}

// A persistent grid of at most 8 workgroups a CU in which every wave takes the same number of
// items (to within one), as the statistics passes size theirs.
unsigned balanced_blocks(int64_t n_items, int num_cus, int per_block) {
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 8 * per_block;
    const int64_t rounds = (n_items + cap - 1) / cap;
    const int64_t takers = (n_items + rounds - 1) / rounds;
    return (unsigned)((takers + per_block - 1) / per_block);
}

// Lanes across a dense row of nvec 16-byte vectors: a power of two, at most 64.
int dense_group(int nvec) {
    int gl = 64;
    if (nvec < 64) {
        gl = 1;
        while (gl < nvec) gl *= 2;
    }
    return gl;
}

}  // namespace

int gather_tile_rows(int layout, int64_t row_bytes) {
    if (layout == kCsr) return kCsrTile;
    // about 64 KiB a tile, a whole number of the rows a wave keeps in flight, 16 .. 1,024 rows
    const int nvec = (int)((row_bytes + 15) / 16);
    const int unit = (64 / dense_group(nvec)) * kGatherRows;
    int64_t rows = (65536 / (row_bytes > 0 ? row_bytes : 16)) / unit * unit;
    if (rows < unit) rows = unit;
    if (rows < 16) rows = 16;
    if (rows > 1024) rows = 1024;
    return (int)rows;
}

int launch_gather_dense(const ChainDesc* descs, const SplitPart* tab, int n_parts, int64_t n_tiles, int tile_rows,
                        int d, int storage, int64_t ld_out, int num_cus, hipStream_t st) {
    if (n_tiles <= 0 || n_parts <= 0) return 0;
    const int vec = storage == 1 ? 4 : 2;
    const int nvec_out = (int)(ld_out / vec);
    const int gl = dense_group(nvec_out);
    const dim3 gr(balanced_blocks(n_tiles, num_cus, kGatherWaves)), bl(kGatherBlock);
    if (storage == 1)
        hipLaunchKernelGGL(gather_dense<float>, gr, bl, 0, st, descs, tab, n_parts, n_tiles, tile_rows, d, gl, nvec_out,
                           ld_out);
    else
        hipLaunchKernelGGL(gather_dense<double>, gr, bl, 0, st, descs, tab, n_parts, n_tiles, tile_rows, d, gl,
                           nvec_out, ld_out);
    return (int)hipGetLastError();
}

int launch_gather_csr(const ChainDesc* descs, const SplitPart* tab, int n_parts, int64_t n_tiles, int storage,
                      int64_t max_nnz, int64_t* tile_sum, int num_cus, hipStream_t st) {
    if (n_parts <= 0) return 0;
    int e = 0;
    const dim3 bl(kGatherBlock);
    const dim3 gr(n_tiles > 0 ? balanced_blocks(n_tiles, num_cus, 1) : 1);
    if (n_tiles > 0) {
        hipLaunchKernelGGL(csr_tile_sums, gr, bl, 0, st, descs, tab, n_parts, n_tiles, tile_sum);
        if ((e = (int)hipGetLastError())) return e;
    }
    hipLaunchKernelGGL(csr_tile_bases, dim3((unsigned)n_parts), bl, 0, st, tab, tile_sum);
    if ((e = (int)hipGetLastError())) return e;
    if (n_tiles <= 0) return 0;
    const int gl = max_nnz <= 16 ? 16 : max_nnz <= 32 ? 32 : 64;
    if (storage == 1)
        hipLaunchKernelGGL(gather_csr<float>, gr, bl, 0, st, descs, tab, n_parts, n_tiles, gl, tile_sum);
    else
        hipLaunchKernelGGL(gather_csr<double>, gr, bl, 0, st, descs, tab, n_parts, n_tiles, gl, tile_sum);
    return (int)hipGetLastError();
}

}  // namespace psgd
