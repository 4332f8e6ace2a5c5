// psgd_forest.hip -- a random-forest classifier over the binned rows of psgd_tree.hip, a group of trees a
// level at a time (psgd_forest_bag_device, psgd_forest_histogram_device, psgd_forest_route_device,
// psgd_forest_predict). include/psgd.h has the definitions; every count is an exact integer. The split pass
// (psgd_forest_best_split_device) is tree_best_split's second instantiation in psgd_tree.hip.
//
// forest_weight: the bag weight of (seed, tree, global row) -- two splitmix64 finalisers and 15 integer
// compares against the caller's thresholds. Recomputed wherever it is needed: nothing of trees x rows is kept.
//
// forest_hist: a work item is (row span, node sub-group [a0, a0 + S), subset chunk [j0, j0 + J)); a workgroup
// of 1,024 lanes, one a CU, keeps in LDS the table [S][J][B][K] uint32, the sub-group's feature subsets
// [S][J], a list of 2,048 entries and a tile of binned rows (16 KiB of row bytes, a power of two of rows):
// up to 156 of the CU's 160 KiB. It walks its span tile by tile and, for every batch of the trees the
// sub-group touches, runs two phases:
//   A  lane (tree, row): slot[t][row] -> the node a = tree_base[t] + slot; when a lies in the sub-group, the
//      label byte and the bag weight w; w > 0 appends one packed entry {row of the tile, a - a0, w, label} to
//      the list (an LDS counter: the order varies, the sums do not).
//   B  lane (entry, j), consecutive lanes along j first: the feature f = subset[a][j] from LDS, the byte
//      tile[row][f] from LDS, one LDS integer add of w at [a - a0][j][bin][label]. The lanes step through
//      (entry, j) by increments, without a division. A wave's 64 adds lie over ~64 / J entries' features:
//      different nodes and features, so different banks; the tile's pitch is padded by 16 bytes so that
//      the same feature of neighbouring rows is not one bank.
// The tile is staged (16-byte loads, as tree_hist reads its vectors) only when some batch of it has an entry,
// once for all trees of the sub-group. Rows wider than the tile (pitch > 16 KiB) are not staged: phase B
// reads their bytes through L2. The item ends by adding its non-zero cells to the compact 64-bit table
// [nodes][m][B][K] with integer atomics. A span has at most 2^28 rows: 15 x 2^28 < 2^32.
//
// forest_route: a lane a row, the trees of the group in a loop (the row's bytes stay in cache between them).
// forest_predict_dense: a lane a row over the trees' concatenated nodes; votes in LDS counters [K][lane].
#include <algorithm>

#include "psgd_device.h"

namespace psgd {
namespace {

constexpr int kForestBlock = 1024;           // lanes of forest_hist
constexpr int kForestList = 2048;            // entries a batch of trees may append (tile rows x trees a batch)
constexpr int kForestTileBytes = 16384;      // row bytes a tile stages
constexpr int kForestTileRows = 256;         // rows a tile at most (8 bits of an entry)
constexpr int64_t kForestItems = 512;        // work items the plan aims at (one workgroup a CU, twice over)
constexpr int kForestSmall = 256;            // lanes of the other kernels

__global__ __launch_bounds__(256) void forest_zero(unsigned long long* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0ull;
}

__device__ __forceinline__ unsigned long long forest_mix(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
constexpr unsigned long long kForestGold = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ unsigned long long forest_key(unsigned long long seed, int64_t tree) {
    return forest_mix(seed + (unsigned long long)(tree + 1) * kForestGold);
}
// 0 .. 15: the thresholds u reaches (g: the row's global index).
__device__ __forceinline__ int forest_weight(const ForestBag& bag, unsigned long long key, int64_t g) {
    const unsigned long long u = forest_mix(key + (unsigned long long)(g + 1) * kForestGold) >> 11;
    int w = 0;
#pragma unroll
    for (int k = 0; k < 15; ++k) w += u >= bag.cut[k] ? 1 : 0;
    return w;
}

__global__ __launch_bounds__(kForestSmall) void forest_bag(ForestBag bag, int n_trees, int64_t n_rows,
                                                            uint8_t* __restrict__ w) {
    const unsigned long long key = forest_key(bag.seed, bag.tree0 + (int64_t)blockIdx.y);
    uint8_t* out = w + (int64_t)blockIdx.y * n_rows;
    for (int64_t row = (int64_t)blockIdx.x * kForestSmall + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * kForestSmall)
        out[row] = (uint8_t)forest_weight(bag, key, bag.row0 + row);
}

// Nodes n0 .. n0 + nn - 1 of the frontier (a node group); hist [nn][m][B][K]. node_tree [A], tree_base
// [G + 1] and sub [A][m] describe the whole frontier; slot [G][slot_ld].
template <bool STAGE>
__global__ __launch_bounds__(kForestBlock) void forest_hist(const uint8_t* __restrict__ bins,
                                                            const uint8_t* __restrict__ labels,
                                                            const int32_t* __restrict__ slot, int64_t slot_ld, int64_t n_rows,
                                                            ForestGeom gm, ForestBag bag,
                                                            const int32_t* __restrict__ node_tree,
                                                            const int32_t* __restrict__ tree_base, int G,
                                                            const int32_t* __restrict__ sub, int n0, int nn,
                                                            unsigned long long* __restrict__ hist,
                                                            unsigned long long* __restrict__ nbad) {
    extern __shared__ __align__(16) unsigned forest_lds[];
    __shared__ unsigned cnt_s;
    const int B = gm.bins, K = gm.classes, BK = B * K, S = gm.sgroup, J = gm.jchunk, m = gm.m, d = gm.d;
    const int cells = S * J * BK;
    unsigned* table = forest_lds;                                    // [S][J][B][K]
    int32_t* sub_s = reinterpret_cast<int32_t*>(table + cells);      // [S][J]
    unsigned* list = forest_lds + gm.list_off;                       // [kForestList]
    uint8_t* tile = reinterpret_cast<uint8_t*>(list + kForestList);               // [tile_rows][pitch + 16]
    const int tid = threadIdx.x;
    int64_t item = blockIdx.x;
    const int jc = (int)(item % gm.n_jchunks);
    item /= gm.n_jchunks;
    const int n_sg = (nn + S - 1) / S;
    const int sg = (int)(item % n_sg);
    const int64_t span = item / n_sg;
    const int a0 = n0 + sg * S;
    const int sn = min(S, n0 + nn - a0);                 // the sub-group's nodes
    const int j0 = jc * J;
    const int Jn = min(J, m - j0);                       // the chunk's subset positions
    for (int i = tid; i < cells; i += kForestBlock) table[i] = 0u;
    for (int i = tid; i < S * J; i += kForestBlock) {
        const int al = i / J, j = i - al * J;
        sub_s[i] = al < sn && j < Jn ? sub[(int64_t)(a0 + al) * m + j0 + j] : -1;
    }
    const int t_lo = max(0, min(G - 1, node_tree[a0]));
    const int t_hi = max(t_lo, min(G - 1, node_tree[a0 + sn - 1]));
    const int TR = gm.tile_rows, lg = gm.tile_log2, TB = kForestList / TR;
    const int pitch = gm.pitch, tp = pitch + 16, pv = pitch >> 4;
    // phase B's walk over (entry, j): this lane's start and its step of kForestBlock positions
    const int e0 = tid / Jn, jj0 = tid - e0 * Jn;
    const int step_e = kForestBlock / Jn, step_j = kForestBlock - step_e * Jn;
    const int64_t r_lo = span * gm.span_rows;
    const int64_t r_hi = min(r_lo + gm.span_rows, n_rows);
    __syncthreads();
    for (int64_t r0 = r_lo; r0 < r_hi; r0 += TR) {
        const int tr = (int)min((int64_t)TR, r_hi - r0);
        if (sg == 0 && jc == 0 && tid < tr && labels[r0 + tid] >= K) atomicAdd(nbad, 1ull);
        bool staged = false;
        for (int tb = t_lo; tb <= t_hi; tb += TB) {
            if (tid == 0) cnt_s = 0u;
            __syncthreads();
            const int nt = min(TB, t_hi - tb + 1);
            for (int u = tid; u < nt * TR; u += kForestBlock) {
                const int rl = u & (TR - 1), t = tb + (u >> lg);
                if (rl >= tr) continue;
                const int64_t row = r0 + rl;
                const int s = slot[(int64_t)t * slot_ld + row];
                const int base = tree_base[t];
                const int al = base + s - a0;
                if (s < 0 || s >= tree_base[t + 1] - base || al < 0 || al >= sn) continue;
                const int lab = labels[row];
                if (lab >= K) continue;
                const int w = forest_weight(bag, forest_key(bag.seed, bag.tree0 + (int64_t)t), bag.row0 + row);
                if (w == 0) continue;
                const unsigned pos = atomicAdd(&cnt_s, 1u);
                list[pos] = (unsigned)rl | ((unsigned)al << 8) | ((unsigned)w << 21) | ((unsigned)lab << 25);
            }
            __syncthreads();
            const int cnt = (int)cnt_s;
            if (cnt > 0) {
                if (STAGE && !staged) {
                    for (int v = tid; v < tr * pv; v += kForestBlock) {
                        const int rl = v / pv, c = v - rl * pv;
                        *reinterpret_cast<uint4*>(tile + rl * tp + 16 * c) =
                            *reinterpret_cast<const uint4*>(bins + (r0 + rl) * pitch + 16 * c);
                    }
                    staged = true;
                    __syncthreads();
                }
                int e = e0, j = jj0;
                while (e < cnt) {
                    const unsigned ent = list[e];
                    const int rl = (int)(ent & 255u), al = (int)((ent >> 8) & 8191u);
                    const unsigned w = (ent >> 21) & 15u;
                    const int lab = (int)(ent >> 25);
                    const int f = sub_s[al * J + j];
                    if ((unsigned)f < (unsigned)d) {
                        const int b = STAGE ? (int)tile[rl * tp + f] : (int)bins[(r0 + rl) * pitch + f];
                        if (b < B) atomicAdd(table + (al * J + j) * BK + b * K + lab, w);
                    }
                    j += step_j;
                    e += step_e;
                    if (j >= Jn) {
                        j -= Jn;
                        ++e;
                    }
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int i = tid; i < cells; i += kForestBlock) {
        const unsigned c = table[i];
        if (!c) continue;
        const int al = i / (J * BK);
        const int rem = i - al * J * BK;
        const int j = rem / BK;
        if (al < sn && j < Jn)
            atomicAdd(hist + ((int64_t)(a0 - n0 + al) * m + j0 + j) * BK + (rem - j * BK), (unsigned long long)c);
    }
}

// table [A][4] = {feature (-1: a leaf), bin, left, right}: the children are slots of the tree's next frontier.
__global__ __launch_bounds__(kForestSmall) void forest_route(const uint8_t* __restrict__ bins, int pitch, int64_t n_rows,
                                                              const int32_t* __restrict__ table,
                                                              const int32_t* __restrict__ tree_base, int G,
                                                              int32_t* __restrict__ slot, int64_t slot_ld) {
    for (int64_t row = (int64_t)blockIdx.x * kForestSmall + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * kForestSmall) {
        const uint8_t* br = bins + row * pitch;
        for (int t = 0; t < G; ++t) {
            const int s = slot[(int64_t)t * slot_ld + row];
            if (s < 0) continue;
            int next = -1;
            const int base = tree_base[t];
            if (s < tree_base[t + 1] - base) {
                const int4 q = *reinterpret_cast<const int4*>(table + 4 * (int64_t)(base + s));
                if (q.x >= 0 && q.x < pitch) next = (int)br[q.x] <= q.y ? q.z : q.w;
            }
            slot[(int64_t)t * slot_ld + row] = next;
        }
    }
}

struct ForestNode {    // 24 bytes; left and right index the concatenated array
    double threshold;
    int32_t feature;   // -1: a leaf, whose class is `left`
    int32_t left;
    int32_t right, pad;
};
static_assert(sizeof(ForestNode) == 24, "ForestNode");

// root [n_trees]: a tree's first node. The host has checked feature < d and node < left, right < the tree's end.
template <typename S>
__global__ __launch_bounds__(kForestSmall) void forest_predict_dense(const ChainDesc* __restrict__ descs,
                                                                      const int64_t* __restrict__ row_off, int P,
                                                                      int64_t n_rows, const ForestNode* __restrict__ nodes,
                                                                      const int32_t* __restrict__ root, int n_trees, int K,
                                                                      int32_t* __restrict__ cls, int32_t* __restrict__ votes) {
    __shared__ int vote_s[kTreeMaxClasses * kForestSmall];   // [class][lane]
    int* mine = vote_s + threadIdx.x;
    for (int64_t row = (int64_t)blockIdx.x * kForestSmall + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * kForestSmall) {
        int lo = 0, hi = P;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (row_off[mid] <= row) lo = mid; else hi = mid;
        }
        const ChainDesc dsc = descs[lo];
        const S* xr = reinterpret_cast<const S*>(dsc.x) + (row - row_off[lo]) * dsc.ld;
        for (int c = 0; c < K; ++c) mine[c * kForestSmall] = 0;
        for (int t = 0; t < n_trees; ++t) {
            ForestNode nd = nodes[root[t]];
            while (nd.feature >= 0) nd = nodes[(double)xr[nd.feature] <= nd.threshold ? nd.left : nd.right];
            if ((unsigned)nd.left < (unsigned)K) mine[nd.left * kForestSmall] += 1;
        }
        int best = 0, bv = mine[0];
        for (int c = 0; c < K; ++c) {
            const int v = mine[c * kForestSmall];
            if (votes) votes[row * K + c] = v;
            if (v > bv) {                                // (strict: a tie goes to the lowest class)
                bv = v;
                best = c;
            }
        }
        cls[row] = best;
    }
}

unsigned forest_blocks(int64_t n, int per, int num_cus) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, (int64_t)num_cus * 8));
}

}  // namespace

ForestGeom forest_geometry(int d, int bins, int classes, int m, int nodes, int64_t n_tiles, int64_t budget) {
    ForestGeom gm{};
    gm.d = d;
    gm.bins = bins;
    gm.classes = classes;
    gm.m = m;
    gm.pitch = 16 * ((d + 15) / 16);
    const int64_t per_node = (int64_t)m * bins * classes * (int64_t)sizeof(int64_t);
    gm.group_nodes = (int32_t)std::max<int64_t>(1, std::min<int64_t>(nodes, budget / per_node));
    gm.n_groups = (nodes + gm.group_nodes - 1) / gm.group_nodes;
    gm.scratch_bytes = gm.group_nodes * per_node;
    // (node, subset position) pairs an item holds: B K cells and one subset entry each
    const int unit = bins * classes + 1;
    const int pairs = kForestLdsCells / unit;            // >= 3: bins classes <= 8,192
    if (m <= pairs) {
        gm.jchunk = m;
        gm.sgroup = std::max(1, std::min(std::min(gm.group_nodes, pairs / m), 8191));
    } else {
        gm.jchunk = pairs;
        gm.sgroup = 1;
    }
    gm.n_jchunks = (m + gm.jchunk - 1) / gm.jchunk;
    gm.n_sgroups = (gm.group_nodes + gm.sgroup - 1) / gm.sgroup;
    // the row tile: a power of two of rows within kForestTileBytes; none when one row exceeds it
    gm.staged = gm.pitch <= kForestTileBytes ? 1 : 0;
    int tr = 1, lg = 0;
    while (2 * tr <= kForestTileRows && (int64_t)2 * tr * gm.pitch <= kForestTileBytes) {
        tr *= 2;
        ++lg;
    }
    gm.tile_rows = tr;
    gm.tile_log2 = lg;
    gm.list_off = 4 * (((int64_t)gm.sgroup * gm.jchunk * unit + 3) / 4);   // (the list and the tile on 16 bytes)
    gm.lds_bytes = (gm.list_off + kForestList) * (int64_t)sizeof(uint32_t) + (gm.staged ? (int64_t)tr * (gm.pitch + 16) : 0);
    const int64_t sub = (int64_t)gm.n_jchunks * gm.n_sgroups;
    const int64_t T = std::max<int64_t>(n_tiles, 1);
    const int64_t want = std::min<int64_t>(T, std::max<int64_t>(1, kForestItems / sub));
    // (15 x a span's rows stay below 2^32: a uint32 cell of the LDS table cannot wrap)
    const int64_t span_tiles = std::min<int64_t>((T + want - 1) / want, (1ll << 28) / kTreeTileRows);
    gm.span_rows = span_tiles * kTreeTileRows;
    gm.n_spans = (T + span_tiles - 1) / span_tiles;
    gm.n_items = gm.n_spans * sub;
    return gm;
}

int launch_forest_bag(const ForestBag& bag, int n_trees, int64_t n_rows, uint8_t* w, int num_cus, hipStream_t st) {
    if (n_rows <= 0) return 0;
    hipLaunchKernelGGL(forest_bag, dim3(forest_blocks(n_rows, kForestSmall, num_cus), (unsigned)n_trees), dim3(kForestSmall), 0,
                       st, bag, n_trees, n_rows, w);
    return (int)hipGetLastError();
}

int launch_forest_hist(const uint8_t* bins, const uint8_t* labels, const int32_t* slot, int64_t slot_ld, int64_t n_rows,
                       const ForestGeom& gm, const ForestBag& bag, const int32_t* node_tree, const int32_t* tree_base,
                       int n_trees, const int32_t* sub, int node0, int n_nodes, int64_t* hist, int64_t* nbad,
                       hipStream_t st) {
    unsigned long long* H = reinterpret_cast<unsigned long long*>(hist);
    const int64_t total = (int64_t)n_nodes * gm.m * gm.bins * gm.classes;
    // the table starts from zero: a kernel, not a memset node, so that a captured level replays
    hipLaunchKernelGGL(forest_zero, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 2048))),
                       dim3(256), 0, st, H, total);
    int e = (int)hipGetLastError();
    if (e || n_rows <= 0) return e;
    const int n_sg = (n_nodes + gm.sgroup - 1) / gm.sgroup;   // (a last group may be short)
    const int64_t items = gm.n_spans * gm.n_jchunks * n_sg;
    auto kern = gm.staged ? forest_hist<true> : forest_hist<false>;
    if (gm.lds_bytes > 64 * 1024) {
        const hipError_t a = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gm.lds_bytes);
        if (a != hipSuccess) return (int)a;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)items), dim3(kForestBlock), (size_t)gm.lds_bytes, st, bins, labels, slot, slot_ld,
                       n_rows, gm, bag, node_tree, tree_base, n_trees, sub, node0, n_nodes, H,
                       reinterpret_cast<unsigned long long*>(nbad));
    return (int)hipGetLastError();
}

int launch_forest_route(const uint8_t* bins, int pitch, int64_t n_rows, const int32_t* table, const int32_t* tree_base,
                        int n_trees, int32_t* slot, int64_t slot_ld, int num_cus, hipStream_t st) {
    if (n_rows <= 0) return 0;
    hipLaunchKernelGGL(forest_route, dim3(forest_blocks(n_rows, kForestSmall, num_cus)), dim3(kForestSmall), 0, st, bins, pitch,
                       n_rows, table, tree_base, n_trees, slot, slot_ld);
    return (int)hipGetLastError();
}

int launch_forest_predict(const ChainDesc* descs, const int64_t* row_off, int n_parts, int64_t n_rows, int storage,
                          const void* nodes, const int32_t* root, int n_trees, int classes, int32_t* cls, int32_t* votes,
                          int num_cus, hipStream_t st) {
    if (n_rows <= 0) return 0;
    const ForestNode* nd = reinterpret_cast<const ForestNode*>(nodes);
    const dim3 grid(forest_blocks(n_rows, kForestSmall, num_cus)), block(kForestSmall);
    if (storage == 1)
        hipLaunchKernelGGL(forest_predict_dense<float>, grid, block, 0, st, descs, row_off, n_parts, n_rows, nd, root, n_trees,
                           classes, cls, votes);
    else
        hipLaunchKernelGGL(forest_predict_dense<double>, grid, block, 0, st, descs, row_off, n_parts, n_rows, nd, root, n_trees,
                           classes, cls, votes);
    return (int)hipGetLastError();
}

}  // namespace psgd
