// psgd_tree.hip -- a decision-tree classifier over the registered dense partitions, level by level
// (psgd_tree_bin_device, psgd_tree_histogram_device, psgd_tree_best_split_device, psgd_tree_route_device,
// psgd_tree_predict). include/psgd.h has the definitions; every count is an exact integer.
//
// tree_bin_dense: a workgroup takes a chunk of features whose thresholds fit 64 KiB of LDS (tp = B - 1
// doubles a feature) and strides over the rows. A lane takes (row, 16 features): it reads the values as
// 16-byte vectors of the storage type (a vector that reaches column d is read element by element below
// d: a zero-copy row's pad is never read), widens each to f64, binary-searches its feature's thresholds
// (bin = the number of thresholds t with x > t) and writes the 16 bytes with one store; bytes of features
// >= d are 0. The lane of a row's first vector also writes the row's label byte (255: not a whole number
// in [0, 255)).
//
// tree_hist: a work item is (row span, feature chunk, slot sub-group); a workgroup of 256 lanes keeps the
// sub-table [copy][slot][feature][bin][class] as uint32 in 64 KiB of LDS at most, so that two workgroups
// share a CU. Lane (row, vector) loads slot[row]; only when the slot lies in the item's sub-group does it
// load the label byte and the 16-byte vector of the row's bins, and issues one LDS integer add a feature.
// The lanes of a step lie along a row's vectors first, so a wave's adds spread over as many features as the
// chunk has vectors; with two copies (gm.repl = 2) odd and even rows add into copies of their own. The item
// ends by adding its non-zero cells (the copies summed) to the global 64-bit table with integer atomics.
// Integers only: exact in any order, the same bits from call to call. The matrix cores have no part in
// this: a one-hot product would spend B K multiplies on what is one add.
//
// tree_best_split: a workgroup a slot, a wave a (slot, feature) at a time. Lane j takes bins j, j + 64, ..:
// per class an inclusive 64-bit integer scan over the wave (carried from 64 bins to the next, the carries in
// LDS) gives L[c]; the classes are walked twice, once for nL and once for the impurities, so nothing is kept
// per class in registers; the gains are fp64 with the classes in index order. Every lane keeps its best candidate (features and
// bins ascend, strict >), the wave's butterfly and then the four waves' pairs apply the tie rule: the
// larger gain, else the lower feature, else the lower bin. One record a slot.
//
// tree_route: a lane a row: slot[r] <- the left or right child's slot from the per-slot table.
//
// tree_predict_dense: a lane a row, the node arrays in LDS while they fit 64 KiB (32 bytes a node), else
// read through L2; at most `depth` scattered loads of the row's features.
//
// The regression tree (psgd_tree_label_range_device, psgd_tree_targets_device, psgd_tree_moments_device,
// psgd_tree_histogram_reg_device, psgd_tree_best_split_reg_device) follows tree_predict_dense below: fixed-point
// targets, node moments, a {count, sum} histogram and the variance split, each described at its kernel.
#include <algorithm>

#include "psgd_device.h"

namespace psgd {
namespace {

constexpr int kTreeBlock = 256;
constexpr int kTreeWaves = kTreeBlock / 64;
constexpr int64_t kTreeItems = 1024;         // work items the histogram's plan aims at (2 a CU, twice over)
constexpr int kTreeThrLds = 8192;            // doubles of thresholds a workgroup of tree_bin_dense stages
constexpr int kTreeNodeLds = 2048;           // nodes tree_predict_dense keeps in LDS (32 bytes each)

__global__ __launch_bounds__(256) void tree_zero(unsigned long long* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0ull;
}

// The row's partition: the last p with row_off[p] <= row (row_off[P] = the rows).
__device__ __forceinline__ int tree_partition(const int64_t* row_off, int P, int64_t row) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (row_off[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
}

// blockIdx.y: the feature chunk (fvec vectors of 16 features); blockIdx.x strides over steps of rows.
template <typename S>
__global__ __launch_bounds__(kTreeBlock) void tree_bin_dense(const ChainDesc* __restrict__ descs,
                                                             const int64_t* __restrict__ row_off, int P, int64_t n_rows,
                                                             int d, int B, int pitch, int fvec,
                                                             const double* __restrict__ thr,
                                                             const int32_t* __restrict__ nbins,
                                                             uint8_t* __restrict__ bins, uint8_t* __restrict__ labels) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    extern __shared__ double tree_thr[];
    const int tp = B - 1;
    const int nvec = pitch >> 4;
    const int v0 = blockIdx.y * fvec;
    const int nv = min(fvec, nvec - v0);                 // the chunk's vectors (>= 1)
    const int f0 = 16 * v0;
    const int nf = min(16 * nv, d - f0);                 // its features (>= 1)
    for (int i = threadIdx.x; i < nf * tp; i += kTreeBlock) tree_thr[i] = thr[(int64_t)f0 * tp + i];
    __syncthreads();
    const int rps = kTreeBlock / nv;                     // rows a step
    const int rin = threadIdx.x / nv, v = threadIdx.x - rin * nv;
    if (rin >= rps) return;
    for (int64_t row = (int64_t)blockIdx.x * rps + rin; row < n_rows; row += (int64_t)gridDim.x * rps) {
        const int p = tree_partition(row_off, P, row);
        const ChainDesc dsc = descs[p];
        const int64_t r = row - row_off[p];
        const S* xr = reinterpret_cast<const S*>(dsc.x) + r * dsc.ld;
        const int fb = f0 + 16 * v;                      // the lane's first feature
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int g = 0; g < 16 / VEC; ++g) {
            const int fg = fb + g * VEC;
            double a[VEC];
            if (fg + VEC <= d) {
                unpack<S, double>(*reinterpret_cast<const V*>(xr + fg), a);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) a[e] = fg + e < d ? (double)xr[fg + e] : 0.0;
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int f = fg + e;
                unsigned b = 0u;
                if (f < d) {
                    const double* t = tree_thr + (f - f0) * tp;
                    int lo = 0, hi = nbins[f] - 1;       // the thresholds of feature f
                    hi = hi < 0 ? 0 : hi > tp ? tp : hi;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (a[e] > t[mid]) lo = mid + 1; else hi = mid;
                    }
                    b = (unsigned)lo;
                }
                const int k = g * VEC + e;
                w[k >> 2] |= b << (8 * (k & 3));
            }
        }
        *reinterpret_cast<uint4*>(bins + row * pitch + 16 * (v0 + v)) = make_uint4(w[0], w[1], w[2], w[3]);
        if (v0 + v == 0) {
            const double y = dsc.y[r];
            labels[row] = y >= 0.0 && y < 255.0 && y == (double)(int)y ? (uint8_t)(int)y : (uint8_t)255;
        }
    }
}

__global__ __launch_bounds__(kTreeBlock, 2) void tree_hist(const uint8_t* __restrict__ bins,
                                                           const uint8_t* __restrict__ labels,
                                                           const int32_t* __restrict__ slot, int64_t n_rows, TreeGeom gm,
                                                           int slot0, int n_slots, unsigned long long* __restrict__ hist,
                                                           unsigned long long* __restrict__ nbad) {
    extern __shared__ unsigned tree_tab[];
    const int B = gm.bins, K = gm.classes, BK = B * K, FC = gm.fchunk, S = gm.sgroup, d = gm.d;
    const int cells = S * FC * BK;                       // one copy (gm.repl cells <= kTreeLdsCells)
    int64_t item = blockIdx.x;
    const int fc = (int)(item % gm.n_fchunks);
    item /= gm.n_fchunks;
    const int sg = (int)(item % gm.n_sgroups);
    const int64_t span = item / gm.n_sgroups;
    for (int i = threadIdx.x; i < cells * gm.repl; i += kTreeBlock) tree_tab[i] = 0u;
    __syncthreads();
    // the chunk's vectors of a row, and the bytes of a vector that belong to it (a chunk of fewer than
    // 16 features is a part of one vector)
    const int nvec = gm.pitch >> 4;
    const bool wide = FC >= 16;
    const int vec0 = wide ? fc * (FC >> 4) : (fc * FC) >> 4;
    const int nv = wide ? min(FC >> 4, nvec - vec0) : 1;
    const int e_lo = wide ? 0 : (fc * FC) & 15, e_hi = wide ? 16 : e_lo + FC;
    const int rps = kTreeBlock / nv;
    const int rin = threadIdx.x / nv, v = threadIdx.x - rin * nv;
    const int sbase = slot0 + sg * S;
    const int sn = min(S, n_slots - sg * S);             // the sub-group's slots
    const int64_t r0 = span * gm.span_rows;
    const int64_t r1 = min(r0 + gm.span_rows, n_rows);
    if (rin < rps) {
        for (int64_t row = r0 + rin; row < r1; row += rps) {
            const int s = slot[row] - sbase;
            if (s < 0 || s >= sn) continue;
            const int lab = labels[row];
            if (lab >= K) {                              // (once a row: the first vector of the first chunk)
                if (fc == 0 && v == 0) atomicAdd(nbad, 1ull);
                continue;
            }
            const uint4 q = *reinterpret_cast<const uint4*>(bins + row * gm.pitch + 16 * (vec0 + v));
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
            unsigned* tab = tree_tab + (gm.repl == 2 && (row & 1) ? cells : 0) + s * FC * BK + lab;
            const int fl0 = 16 * (vec0 + v) - fc * FC;   // the vector's byte 0 as a feature of the chunk
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int b = (int)((w[e >> 2] >> (8 * (e & 3))) & 255u);
                const int fl = fl0 + e;
                if (e >= e_lo && e < e_hi && fc * FC + fl < d && b < B) atomicAdd(tab + fl * BK + b * K, 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += kTreeBlock) {
        const unsigned c = tree_tab[i] + (gm.repl == 2 ? tree_tab[cells + i] : 0u);
        if (!c) continue;
        const int s = i / (FC * BK);
        const int rem = i - s * FC * BK;
        const int fl = rem / BK;
        const int f = fc * FC + fl, gs = sg * S + s;
        if (f < d && gs < n_slots) atomicAdd(hist + ((int64_t)gs * d + f) * BK + (rem - fl * BK), (unsigned long long)c);
    }
}

// One class of imp(v): s accumulates over the classes in index order; v of nn > 0 rows. kind 0 gini, 1 entropy.
__device__ __forceinline__ void tree_imp_add(double& s, double v, double nn, int kind) {
    if (kind == 0) {
        const double q = v / nn;
        s += q * q;
    } else if (v > 0.0) {
        const double q = v / nn;
        s -= q * log(q) / 0.693147180559945309417;
    }
}
__device__ __forceinline__ double tree_imp_end(double s, int kind) { return kind == 0 ? 1.0 - s : s; }

// The wave's inclusive scan of h over its lanes (64-bit integers: exact).
__device__ __forceinline__ unsigned long long tree_scan(unsigned long long h, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long up = __shfl_up(h, off);
        if (lane >= off) h += up;
    }
    return h;
}

struct TreeBest {
    double gain;
    int f, b;
};
// a wins over b: the larger gain, else the lower feature, else the lower bin (f < 0: no candidate).
__device__ __forceinline__ bool tree_better(double ga, int fa, int ba, double gb, int fb, int bb) {
    if (fa < 0) return false;
    if (fb < 0) return true;
    return ga > gb || (ga == gb && (fa < fb || (fa == fb && ba < bb)));
}

// rec [n_slots][6 + 2 K] = {feature (-1: a leaf), bin, threshold, gain, impurity, n, tot[K], L[K]}.
// The classes are walked twice a step of 64 bins -- once for nL, once for the impurities, which need nL --
// with tot and the steps' carries in LDS, so that no per-class array lives in registers.
// SUB (the forest's pass): the slot's table holds d = m positions, position j being feature sub[slot][j]
// (ascending, so the tie rule over positions is the tie rule over features); the record names the feature.
template <bool SUB>
__global__ __launch_bounds__(kTreeBlock) void tree_best_split(const unsigned long long* __restrict__ hist,
                                                              const double* __restrict__ thr,
                                                              const int32_t* __restrict__ nbins,
                                                              const int32_t* __restrict__ sub, int d, int B, int K,
                                                              int kind, double min_inst, double min_gain,
                                                              double* __restrict__ rec) {
    __shared__ double tot_s[kTreeMaxClasses];
    __shared__ double carry_s[kTreeWaves][kTreeMaxClasses];
    __shared__ TreeBest best_s[kTreeWaves];
    __shared__ int win_s[2];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int slot = blockIdx.x;
    const int BK = B * K;
    const unsigned long long* H = hist + (int64_t)slot * d * BK;
    if ((int)threadIdx.x < K) {
        unsigned long long t = 0ull;
        for (int b = 0; b < B; ++b) t += H[b * K + threadIdx.x];
        tot_s[threadIdx.x] = (double)t;
    }
    __syncthreads();
    double n = 0.0, st = 0.0;
    for (int c = 0; c < K; ++c) n += tot_s[c];
    if (n > 0.0)
        for (int c = 0; c < K; ++c) tree_imp_add(st, tot_s[c], n, kind);
    const double imp_t = n > 0.0 ? tree_imp_end(st, kind) : 0.0;
    double* carry = carry_s[wave];                       // (every lane stores the same value: the wave's own)
    double bg = 0.0;
    int bf = -1, bb = -1;
    const int32_t* feat = SUB ? sub + (int64_t)slot * d : nullptr;
    for (int f = wave; f < d; f += kTreeWaves) {
        int ncand = nbins[SUB ? feat[f] : f] - 1;        // candidates: bins 0 .. nb_f - 2
        ncand = ncand > B - 1 ? B - 1 : ncand;
        const unsigned long long* Hf = H + (int64_t)f * BK;
        for (int c = 0; c < K; ++c) carry[c] = 0.0;
        for (int b0 = 0; b0 < ncand; b0 += 64) {         // (uniform over the wave)
            const int b = b0 + lane;
            double nL = 0.0;
            for (int c = 0; c < K; ++c)                  // (whole numbers below 2^53: exact)
                nL += carry[c] + (double)tree_scan(b < ncand ? Hf[b * K + c] : 0ull, lane);
            const double nR = n - nL;
            const bool valid = b < ncand && nL >= min_inst && nR >= min_inst && nL > 0.0 && nR > 0.0;
            const double dl = valid ? nL : 1.0, dr = valid ? nR : 1.0;
            double sl = 0.0, sr = 0.0;
            for (int c = 0; c < K; ++c) {
                const unsigned long long h = tree_scan(b < ncand ? Hf[b * K + c] : 0ull, lane);
                const double Lc = carry[c] + (double)h;
                tree_imp_add(sl, Lc, dl, kind);
                tree_imp_add(sr, tot_s[c] - Lc, dr, kind);
                carry[c] += (double)__shfl(h, 63);
            }
            if (valid) {
                const double gain = imp_t - (nL / n) * tree_imp_end(sl, kind) - (nR / n) * tree_imp_end(sr, kind);
                if (bf < 0 || gain > bg) {
                    bg = gain;
                    bf = f;
                    bb = b;
                }
            }
        }
    }
    for (int off = 1; off < 64; off <<= 1) {
        const double pg = __shfl_xor(bg, off);
        const int pf = __shfl_xor(bf, off), pb = __shfl_xor(bb, off);
        if (tree_better(pg, pf, pb, bg, bf, bb)) {
            bg = pg;
            bf = pf;
            bb = pb;
        }
    }
    if (lane == 0) best_s[wave] = TreeBest{bg, bf, bb};
    __syncthreads();
    double* out = rec + (int64_t)slot * (6 + 2 * K);
    if (threadIdx.x == 0) {
        TreeBest w = best_s[0];
        for (int i = 1; i < kTreeWaves; ++i)
            if (tree_better(best_s[i].gain, best_s[i].f, best_s[i].b, w.gain, w.f, w.b)) w = best_s[i];
        const bool split = w.f >= 0 && w.gain > 0.0 && w.gain >= min_gain;
        win_s[0] = split ? w.f : -1;
        win_s[1] = split ? w.b : -1;
        const int wf = split && SUB ? feat[w.f] : w.f;
        out[0] = split ? (double)wf : -1.0;
        out[1] = split ? (double)w.b : -1.0;
        out[2] = split ? thr[(int64_t)wf * (B - 1) + w.b] : 0.0;
        out[3] = w.f >= 0 ? w.gain : 0.0;
        out[4] = imp_t;
        out[5] = n;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const int c = threadIdx.x, f = win_s[0], bw = win_s[1];
        unsigned long long l = 0ull;
        if (f >= 0)
            for (int b = 0; b <= bw; ++b) l += H[(int64_t)f * BK + b * K + c];
        out[6 + c] = tot_s[c];
        out[6 + K + c] = (double)l;
    }
}

// table [n_table][4] = {feature (-1: a leaf), bin, left slot, right slot}.
__global__ __launch_bounds__(kTreeBlock) void tree_route(const uint8_t* __restrict__ bins, int pitch, int64_t n_rows,
                                                         const int32_t* __restrict__ table, int n_table,
                                                         int32_t* __restrict__ slot) {
    for (int64_t row = (int64_t)blockIdx.x * kTreeBlock + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * kTreeBlock) {
        const int s = slot[row];
        if (s < 0) continue;
        int next = -1;
        if (s < n_table) {
            const int4 t = *reinterpret_cast<const int4*>(table + 4 * s);
            if (t.x >= 0 && t.x < pitch) next = (int)bins[row * pitch + t.x] <= t.y ? t.z : t.w;
        }
        slot[row] = next;
    }
}

struct TreeNode {      // 32 bytes
    double threshold, prob;
    int32_t feature, left, right, pred;
};

// nodes: the host has checked feature < d and node < left, right < n_nodes (the walk ends).
template <typename S, bool LDSN>
__global__ __launch_bounds__(kTreeBlock) void tree_predict_dense(const ChainDesc* __restrict__ descs,
                                                                 const int64_t* __restrict__ row_off, int P,
                                                                 int64_t n_rows, const TreeNode* __restrict__ nodes,
                                                                 int n_nodes, int32_t* __restrict__ cls,
                                                                 double* __restrict__ prob) {
    __shared__ TreeNode nd_s[LDSN ? kTreeNodeLds : 1];
    if constexpr (LDSN) {
        for (int i = threadIdx.x; i < n_nodes; i += kTreeBlock) nd_s[i] = nodes[i];
        __syncthreads();
    }
    const TreeNode* nd = LDSN ? nd_s : nodes;
    for (int64_t row = (int64_t)blockIdx.x * kTreeBlock + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * kTreeBlock) {
        const int p = tree_partition(row_off, P, row);
        const ChainDesc dsc = descs[p];
        const S* xr = reinterpret_cast<const S*>(dsc.x) + (row - row_off[p]) * dsc.ld;
        TreeNode t = nd[0];
        while (t.feature >= 0) t = nd[(double)xr[t.feature] <= t.threshold ? t.left : t.right];
        cls[row] = t.pred;
        if (prob) prob[row] = t.prob;
    }
}

// ---- regression: fixed-point targets, node moments, {count, sum} histograms, variance gains ----

// The order-preserving 64-bit image of a double: a < b exactly when key(a) < key(b) as unsigned integers.
__device__ __forceinline__ unsigned long long tree_key(double y) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(y);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ bool tree_finite(double y) {
    return ((unsigned long long)__double_as_longlong(y) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
// Row `row`'s label: the registered one, or flat[row] when the caller passes labels of its own.
__device__ __forceinline__ double tree_label(const ChainDesc* descs, const int64_t* row_off, int P, const double* flat,
                                             int64_t row) {
    if (flat) return flat[row];
    const int p = tree_partition(row_off, P, row);
    return descs[p].y[row - row_off[p]];
}

__global__ void tree_range_init(unsigned long long* range) {
    range[0] = ~0ull;
    range[1] = 0ull;
    range[2] = 0ull;
}

// range = {min key, max key, labels that are NaN or infinite}: a lane a row, the wave by butterfly, the four
// waves in LDS, then three integer atomics a workgroup -- integer min and max are exact in any order.
__global__ __launch_bounds__(kTreeBlock) void tree_label_range(const ChainDesc* __restrict__ descs,
                                                               const int64_t* __restrict__ row_off, int P,
                                                               const double* __restrict__ flat, int64_t n_rows,
                                                               unsigned long long* __restrict__ range) {
    __shared__ unsigned long long part_s[kTreeWaves][3];
    unsigned long long lo = ~0ull, hi = 0ull, bad = 0ull;
    for (int64_t row = (int64_t)blockIdx.x * kTreeBlock + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * kTreeBlock) {
        const double y = tree_label(descs, row_off, P, flat, row);
        if (!tree_finite(y)) {
            ++bad;
            continue;
        }
        const unsigned long long k = tree_key(y);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
        bad += __shfl_xor(bad, off);
    }
    if ((threadIdx.x & 63) == 0) {
        part_s[threadIdx.x >> 6][0] = lo;
        part_s[threadIdx.x >> 6][1] = hi;
        part_s[threadIdx.x >> 6][2] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kTreeWaves; ++w) {
            lo = part_s[w][0] < lo ? part_s[w][0] : lo;
            hi = part_s[w][1] > hi ? part_s[w][1] : hi;
            bad += part_s[w][2];
        }
        if (lo <= hi) {
            atomicMin(range, lo);
            atomicMax(range + 1, hi);
        }
        if (bad) atomicAdd(range + 2, bad);
    }
}

// q[row] = rint((y - ymin) 2^s): one rounded subtraction, an exact scaling, ties to even. 0 for a bad label.
__global__ __launch_bounds__(kTreeBlock) void tree_targets(const ChainDesc* __restrict__ descs,
                                                           const int64_t* __restrict__ row_off, int P,
                                                           const double* __restrict__ flat, int64_t n_rows, double ymin,
                                                           int s, uint32_t* __restrict__ q) {
    for (int64_t row = (int64_t)blockIdx.x * kTreeBlock + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * kTreeBlock) {
        const double y = tree_label(descs, row_off, P, flat, row);
        const double t = tree_finite(y) ? rint(ldexp(y - ymin, s)) : 0.0;
        q[row] = t >= 0.0 && t <= 1073741824.0 ? (uint32_t)t : 0u;
    }
}

// The wave's sum of v (64-bit integers).
__device__ __forceinline__ unsigned long long tree_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

// One slot's {n, S, sum(q^2 >> 30), sum(q^2 & (2^30 - 1))}, added into the workgroup's table in LDS.
__device__ __forceinline__ void tree_mom_flush(unsigned long long* tab, int s, const unsigned long long (&a)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (a[k]) atomicAdd(tab + 4 * s + k, a[k]);
}

// mom [n_slots][4] (zeroed by the launch): blockIdx.x a span of rows, blockIdx.y a sub-group of kTreeMomSlots
// slots. A lane keeps the four sums of its current slot in registers and adds them to the LDS table when its
// slot changes. At the end a wave whose lanes all hold one slot (the root, a shallow level of sorted rows)
// adds them up by butterfly and issues four LDS adds; any other wave's lanes add their own. One global
// integer atomic a (workgroup, slot, member) that is not zero.
__global__ __launch_bounds__(kTreeBlock) void tree_moments(const uint32_t* __restrict__ q, const int32_t* __restrict__ slot,
                                                           int64_t n_rows, int64_t span_rows, int slot0, int n_slots,
                                                           unsigned long long* __restrict__ mom) {
    __shared__ unsigned long long mom_s[4 * kTreeMomSlots];
    const int g0 = blockIdx.y * kTreeMomSlots;
    const int sbase = slot0 + g0;
    const int sn = min(kTreeMomSlots, n_slots - g0);
    for (int i = threadIdx.x; i < 4 * sn; i += kTreeBlock) mom_s[i] = 0ull;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * span_rows;
    const int64_t r1 = min(r0 + span_rows, n_rows);
    int cur = -1;
    unsigned long long a[4] = {0ull, 0ull, 0ull, 0ull};
    for (int64_t row = r0 + threadIdx.x; row < r1; row += kTreeBlock) {
        const int s = slot[row] - sbase;
        if (s < 0 || s >= sn) continue;
        if (s != cur) {
            if (cur >= 0) tree_mom_flush(mom_s, cur, a);
            cur = s;
            a[0] = a[1] = a[2] = a[3] = 0ull;
        }
        const unsigned long long t = q[row], t2 = t * t;   // (t <= 2^30: t2 <= 2^60)
        a[0] += 1ull;
        a[1] += t;
        a[2] += t2 >> 30;
        a[3] += t2 & ((1ull << 30) - 1ull);
    }
    const int first = __shfl(cur, 0);
    if (__all(cur == first)) {
        if (first >= 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = tree_wave_sum(a[k]);
            if ((threadIdx.x & 63) == 0) tree_mom_flush(mom_s, first, a);
        }
    } else if (cur >= 0) {
        tree_mom_flush(mom_s, cur, a);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * sn; i += kTreeBlock) {
        const unsigned long long v = mom_s[i];
        if (v) atomicAdd(mom + 4 * (int64_t)g0 + i, v);
    }
}

// tree_hist's work split, row reads and part-vector chunks with a cell of {uint32 count, 64-bit sum of the
// rows' targets}: the sums [copy][slot][feature][bin] first in LDS, the counts after them (12 bytes a cell,
// gm.repl cells <= kTreeRegLdsCells). A lane issues one 32-bit and one native 64-bit LDS integer add a
// feature: eight targets near 2^30 already pass a uint32. hist [n_slots][d][bins][2] = {count, sum}.
__global__ __launch_bounds__(kTreeBlock, 2) void tree_hist_reg(const uint8_t* __restrict__ bins,
                                                               const uint32_t* __restrict__ q,
                                                               const int32_t* __restrict__ slot, int64_t n_rows,
                                                               TreeGeom gm, int slot0, int n_slots,
                                                               unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned long long tree_sum[];
    const int B = gm.bins, FC = gm.fchunk, S = gm.sgroup, d = gm.d;
    const int cells = S * FC * B;                        // one copy
    unsigned* tree_cnt = reinterpret_cast<unsigned*>(tree_sum + cells * gm.repl);
    int64_t item = blockIdx.x;
    const int fc = (int)(item % gm.n_fchunks);
    item /= gm.n_fchunks;
    const int sg = (int)(item % gm.n_sgroups);
    const int64_t span = item / gm.n_sgroups;
    for (int i = threadIdx.x; i < cells * gm.repl; i += kTreeBlock) {
        tree_sum[i] = 0ull;
        tree_cnt[i] = 0u;
    }
    __syncthreads();
    const int nvec = gm.pitch >> 4;
    const bool wide = FC >= 16;
    const int vec0 = wide ? fc * (FC >> 4) : (fc * FC) >> 4;
    const int nv = wide ? min(FC >> 4, nvec - vec0) : 1;
    const int e_lo = wide ? 0 : (fc * FC) & 15, e_hi = wide ? 16 : e_lo + FC;
    const int rps = kTreeBlock / nv;
    const int rin = threadIdx.x / nv, v = threadIdx.x - rin * nv;
    const int sbase = slot0 + sg * S;
    const int sn = min(S, n_slots - sg * S);
    const int64_t r0 = span * gm.span_rows;
    const int64_t r1 = min(r0 + gm.span_rows, n_rows);
    if (rin < rps) {
        for (int64_t row = r0 + rin; row < r1; row += rps) {
            const int s = slot[row] - sbase;
            if (s < 0 || s >= sn) continue;
            const unsigned long long t = q[row];
            const uint4 w4 = *reinterpret_cast<const uint4*>(bins + row * gm.pitch + 16 * (vec0 + v));
            const unsigned w[4] = {w4.x, w4.y, w4.z, w4.w};
            const int base = (gm.repl == 2 && (row & 1) ? cells : 0) + s * FC * B;
            const int fl0 = 16 * (vec0 + v) - fc * FC;   // the vector's byte 0 as a feature of the chunk
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int b = (int)((w[e >> 2] >> (8 * (e & 3))) & 255u);
                const int fl = fl0 + e;
                if (e >= e_lo && e < e_hi && fc * FC + fl < d && b < B) {
                    atomicAdd(tree_cnt + base + fl * B + b, 1u);
                    atomicAdd(tree_sum + base + fl * B + b, t);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += kTreeBlock) {
        const unsigned c = tree_cnt[i] + (gm.repl == 2 ? tree_cnt[cells + i] : 0u);
        if (!c) continue;
        const unsigned long long sum = tree_sum[i] + (gm.repl == 2 ? tree_sum[cells + i] : 0ull);
        const int s = i / (FC * B);
        const int rem = i - s * FC * B;
        const int fl = rem / B;
        const int f = fc * FC + fl, gs = sg * S + s;
        if (f < d && gs < n_slots) {
            unsigned long long* cell = hist + 2 * (((int64_t)gs * d + f) * B + (rem - fl * B));
            atomicAdd(cell, (unsigned long long)c);
            if (sum) atomicAdd(cell + 1, sum);
        }
    }
}

// rec [n_slots][4] = {feature (-1: a leaf), bin, threshold, gain}. The slot's n and S come from its moments;
// a wave takes a feature, lane j bins j, j + 64, ..: exact inclusive scans of the counts and of the sums,
// carried from 64 bins to the next in registers, give nL and SL, and nR = n - nL, SR = S - SL as integers.
// gain = ((SL^2 / nL + SR^2 / nR - S^2 / n) / n) 2^-2s in fp64; the candidates, the validity and the tie rule
// are tree_best_split's.
__global__ __launch_bounds__(kTreeBlock) void tree_best_split_reg(const unsigned long long* __restrict__ hist,
                                                                  const long long* __restrict__ mom,
                                                                  const double* __restrict__ thr,
                                                                  const int32_t* __restrict__ nbins, int d, int B, int s,
                                                                  long long min_inst, double min_gain,
                                                                  double* __restrict__ rec) {
    __shared__ TreeBest best_s[kTreeWaves];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int slot = blockIdx.x;
    const unsigned long long* H = hist + (int64_t)slot * d * B * 2;
    const long long n = mom[4 * (int64_t)slot], S = mom[4 * (int64_t)slot + 1];
    const double dn = (double)n;
    const double parent = ((double)S * (double)S) / dn;
    double bg = 0.0;
    int bf = -1, bb = -1;
    for (int f = wave; f < d; f += kTreeWaves) {
        int ncand = nbins[f] - 1;                        // candidates: bins 0 .. nb_f - 2
        ncand = ncand > B - 1 ? B - 1 : ncand;
        const unsigned long long* Hf = H + (int64_t)f * B * 2;
        unsigned long long cn = 0ull, cs = 0ull;
        for (int b0 = 0; b0 < ncand; b0 += 64) {         // (uniform over the wave)
            const int b = b0 + lane;
            const unsigned long long hn = tree_scan(b < ncand ? Hf[2 * b] : 0ull, lane);
            const unsigned long long hs = tree_scan(b < ncand ? Hf[2 * b + 1] : 0ull, lane);
            const long long nL = (long long)(cn + hn), SL = (long long)(cs + hs);
            const long long nR = n - nL, SR = S - SL;
            if (b < ncand && nL >= min_inst && nR >= min_inst && nL > 0 && nR > 0) {
                const double dl = (double)SL, dr = (double)SR;
                const double gain = ldexp(((dl * dl) / (double)nL + (dr * dr) / (double)nR - parent) / dn, -2 * s);
                if (bf < 0 || gain > bg) {
                    bg = gain;
                    bf = f;
                    bb = b;
                }
            }
            cn += __shfl(hn, 63);
            cs += __shfl(hs, 63);
        }
    }
    for (int off = 1; off < 64; off <<= 1) {
        const double pg = __shfl_xor(bg, off);
        const int pf = __shfl_xor(bf, off), pb = __shfl_xor(bb, off);
        if (tree_better(pg, pf, pb, bg, bf, bb)) {
            bg = pg;
            bf = pf;
            bb = pb;
        }
    }
    if (lane == 0) best_s[wave] = TreeBest{bg, bf, bb};
    __syncthreads();
    if (threadIdx.x == 0) {
        TreeBest w = best_s[0];
        for (int i = 1; i < kTreeWaves; ++i)
            if (tree_better(best_s[i].gain, best_s[i].f, best_s[i].b, w.gain, w.f, w.b)) w = best_s[i];
        const bool split = w.f >= 0 && w.gain > 0.0 && w.gain >= min_gain;
        double* out = rec + 4 * (int64_t)slot;
        out[0] = split ? (double)w.f : -1.0;
        out[1] = split ? (double)w.b : -1.0;
        out[2] = split ? thr[(int64_t)w.f * (B - 1) + w.b] : 0.0;
        out[3] = w.f >= 0 ? w.gain : 0.0;
    }
}

unsigned tree_blocks(int64_t n, int per, int num_cus) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, (int64_t)num_cus * 8));
}

}  // namespace

TreeGeom tree_geometry(int d, int bins, int classes, int slots, int64_t n_tiles, int64_t budget, int repl) {
    TreeGeom gm{};
    gm.d = d;
    gm.bins = bins;
    gm.classes = classes;
    gm.pitch = 16 * ((d + 15) / 16);
    const int nvec = gm.pitch / 16;
    // the frontier in groups whose 64-bit tables fit the budget
    // (classes 0: the regression table, a cell {count, sum} of 2 x 64 bits, 12 bytes in LDS)
    const bool reg = classes == 0;
    const int64_t per_slot = (int64_t)d * bins * (reg ? 2 : classes) * (int64_t)sizeof(int64_t);
    gm.group_slots = (int32_t)std::max<int64_t>(1, std::min<int64_t>(slots, budget / per_slot));
    gm.n_groups = (slots + gm.group_slots - 1) / gm.group_slots;
    gm.scratch_bytes = gm.group_slots * per_slot;
    // the sub-table of an item: whole vectors of 16 features first, then slots, then a second copy
    // when one is asked for (repl 2) or comes free (repl 0: every feature and slot of the group fit twice)
    const int cells_f = reg ? bins : bins * classes;
    const int lds_cells = reg ? kTreeRegLdsCells : kTreeLdsCells;
    const int cap = repl == 2 ? lds_cells / 2 : lds_cells;
    if (16 * cells_f <= cap) {
        const int units = cap / (16 * cells_f);
        const int fv = std::min(units, nvec);
        gm.fchunk = 16 * fv;
        gm.sgroup = std::max(1, std::min(gm.group_slots, units / fv));
    } else {
        int fc = 1;
        while (2 * fc * cells_f <= cap) fc *= 2;   // (bins classes <= 8,192: one feature fits either cap)
        gm.fchunk = fc;
        gm.sgroup = 1;
    }
    const int64_t one = (int64_t)gm.sgroup * gm.fchunk * cells_f;
    gm.repl = repl == 2 || (repl == 0 && 2 * one <= lds_cells) ? 2 : 1;
    gm.lds_bytes = gm.repl * one * (int64_t)(reg ? sizeof(uint32_t) + sizeof(uint64_t) : sizeof(uint32_t));
    gm.n_fchunks = gm.fchunk >= 16 ? (nvec + gm.fchunk / 16 - 1) / (gm.fchunk / 16) : (d + gm.fchunk - 1) / gm.fchunk;
    gm.n_sgroups = (gm.group_slots + gm.sgroup - 1) / gm.sgroup;
    const int64_t sub = (int64_t)gm.n_fchunks * gm.n_sgroups;
    const int64_t T = std::max<int64_t>(n_tiles, 1);
    const int64_t want = std::min<int64_t>(T, std::max<int64_t>(1, kTreeItems / sub));
    // (a span's rows stay below 2^32: a uint32 cell of the LDS table cannot wrap)
    const int64_t span_tiles = std::min<int64_t>((T + want - 1) / want, (1ll << 32) / kTreeTileRows - 1);
    gm.span_rows = span_tiles * kTreeTileRows;
    gm.n_spans = (T + span_tiles - 1) / span_tiles;
    gm.n_items = gm.n_spans * sub;
    return gm;
}

int launch_tree_bin(const ChainDesc* descs, const int64_t* row_off, int n_parts, int64_t n_rows, int storage, int d,
                    int bins, const double* thr, const int32_t* nbins, uint8_t* out, uint8_t* labels, int num_cus,
                    hipStream_t st) {
    if (n_rows <= 0) return 0;
    const int pitch = 16 * ((d + 15) / 16), nvec = pitch / 16, tp = bins - 1;
    const int fvec = std::max(1, std::min(std::min(nvec, kTreeBlock), kTreeThrLds / (16 * std::max(tp, 1))));
    const int chunks = (nvec + fvec - 1) / fvec;
    const size_t lds = (size_t)16 * fvec * std::max(tp, 1) * sizeof(double);
    const int rps = kTreeBlock / std::min(fvec, nvec);
    const dim3 grid(tree_blocks(n_rows, rps, num_cus), (unsigned)chunks);
    if (storage == 1)
        hipLaunchKernelGGL(tree_bin_dense<float>, grid, dim3(kTreeBlock), lds, st, descs, row_off, n_parts, n_rows, d, bins,
                           pitch, fvec, thr, nbins, out, labels);
    else
        hipLaunchKernelGGL(tree_bin_dense<double>, grid, dim3(kTreeBlock), lds, st, descs, row_off, n_parts, n_rows, d, bins,
                           pitch, fvec, thr, nbins, out, labels);
    return (int)hipGetLastError();
}

int launch_tree_hist(const uint8_t* bins, const uint8_t* labels, const int32_t* slot, int64_t n_rows, const TreeGeom& gm,
                     int slot0, int n_slots, int64_t* hist, int64_t* nbad, hipStream_t st) {
    unsigned long long* H = reinterpret_cast<unsigned long long*>(hist);
    const int64_t total = (int64_t)n_slots * gm.d * gm.bins * gm.classes;
    // the table starts from zero: a kernel, not a memset node, so that a captured level replays
    hipLaunchKernelGGL(tree_zero, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 2048))),
                       dim3(256), 0, st, H, total);
    int e = (int)hipGetLastError();
    if (e || n_rows <= 0) return e;
    const int n_sg = (n_slots + gm.sgroup - 1) / gm.sgroup;   // (a last group may be short)
    TreeGeom g = gm;
    g.n_sgroups = n_sg;
    const int64_t items = g.n_spans * g.n_fchunks * n_sg;
    hipLaunchKernelGGL(tree_hist, dim3((unsigned)items), dim3(kTreeBlock), (size_t)g.lds_bytes, st, bins, labels, slot,
                       n_rows, g, slot0, n_slots, H, reinterpret_cast<unsigned long long*>(nbad));
    return (int)hipGetLastError();
}

int launch_tree_best_split(const int64_t* hist, const double* thr, const int32_t* nbins, int d, int bins, int classes,
                           int n_slots, int impurity, double min_inst, double min_gain, double* rec, hipStream_t st) {
    const unsigned long long* H = reinterpret_cast<const unsigned long long*>(hist);
    hipLaunchKernelGGL(tree_best_split<false>, dim3((unsigned)n_slots), dim3(kTreeBlock), 0, st, H, thr, nbins,
                       (const int32_t*)nullptr, d, bins, classes, impurity, min_inst, min_gain, rec);
    return (int)hipGetLastError();
}

int launch_forest_best_split(const int64_t* hist, const double* thr, const int32_t* nbins, const int32_t* sub, int m,
                             int bins, int classes, int n_nodes, int impurity, double min_inst, double min_gain,
                             double* rec, hipStream_t st) {
    const unsigned long long* H = reinterpret_cast<const unsigned long long*>(hist);
    hipLaunchKernelGGL(tree_best_split<true>, dim3((unsigned)n_nodes), dim3(kTreeBlock), 0, st, H, thr, nbins, sub, m, bins,
                       classes, impurity, min_inst, min_gain, rec);
    return (int)hipGetLastError();
}

int launch_tree_route(const uint8_t* bins, int pitch, int64_t n_rows, const int32_t* table, int n_table, int32_t* slot,
                      int num_cus, hipStream_t st) {
    if (n_rows <= 0) return 0;
    hipLaunchKernelGGL(tree_route, dim3(tree_blocks(n_rows, kTreeBlock, num_cus)), dim3(kTreeBlock), 0, st, bins, pitch,
                       n_rows, table, n_table, slot);
    return (int)hipGetLastError();
}

int launch_tree_predict(const ChainDesc* descs, const int64_t* row_off, int n_parts, int64_t n_rows, int storage,
                        const void* nodes, int n_nodes, int32_t* cls, double* prob, int num_cus, hipStream_t st) {
    if (n_rows <= 0) return 0;
    const TreeNode* nd = reinterpret_cast<const TreeNode*>(nodes);
    const dim3 grid(tree_blocks(n_rows, kTreeBlock, num_cus)), block(kTreeBlock);
    const bool lds = n_nodes <= kTreeNodeLds;
    if (storage == 1) {
        if (lds) hipLaunchKernelGGL((tree_predict_dense<float, true>), grid, block, 0, st, descs, row_off, n_parts, n_rows, nd, n_nodes, cls, prob);
        else hipLaunchKernelGGL((tree_predict_dense<float, false>), grid, block, 0, st, descs, row_off, n_parts, n_rows, nd, n_nodes, cls, prob);
    } else {
        if (lds) hipLaunchKernelGGL((tree_predict_dense<double, true>), grid, block, 0, st, descs, row_off, n_parts, n_rows, nd, n_nodes, cls, prob);
        else hipLaunchKernelGGL((tree_predict_dense<double, false>), grid, block, 0, st, descs, row_off, n_parts, n_rows, nd, n_nodes, cls, prob);
    }
    return (int)hipGetLastError();
}

int launch_tree_label_range(const ChainDesc* descs, const int64_t* row_off, int n_parts, const double* flat, int64_t n_rows,
                            uint64_t* range, int num_cus, hipStream_t st) {
    unsigned long long* R = reinterpret_cast<unsigned long long*>(range);
    hipLaunchKernelGGL(tree_range_init, dim3(1), dim3(1), 0, st, R);
    int e = (int)hipGetLastError();
    if (e || n_rows <= 0) return e;
    hipLaunchKernelGGL(tree_label_range, dim3(tree_blocks(n_rows, kTreeBlock, num_cus)), dim3(kTreeBlock), 0, st, descs,
                       row_off, n_parts, flat, n_rows, R);
    return (int)hipGetLastError();
}

int launch_tree_targets(const ChainDesc* descs, const int64_t* row_off, int n_parts, const double* flat, int64_t n_rows,
                        double ymin, int s, uint32_t* q, int num_cus, hipStream_t st) {
    if (n_rows <= 0) return 0;
    hipLaunchKernelGGL(tree_targets, dim3(tree_blocks(n_rows, kTreeBlock, num_cus)), dim3(kTreeBlock), 0, st, descs, row_off,
                       n_parts, flat, n_rows, ymin, s, q);
    return (int)hipGetLastError();
}

int launch_tree_moments(const uint32_t* q, const int32_t* slot, int64_t n_rows, int slot0, int n_slots, int64_t* mom,
                        int num_cus, hipStream_t st) {
    unsigned long long* M = reinterpret_cast<unsigned long long*>(mom);
    const int64_t total = 4 * (int64_t)n_slots;
    hipLaunchKernelGGL(tree_zero, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 2048))),
                       dim3(256), 0, st, M, total);
    int e = (int)hipGetLastError();
    if (e || n_rows <= 0) return e;
    // spans of whole tiles, about four a CU; every sub-group of kTreeMomSlots slots reads the spans again
    const int64_t T = (n_rows + kTreeTileRows - 1) / kTreeTileRows;
    const int64_t want = std::min<int64_t>(T, (int64_t)num_cus * 4);
    const int64_t span_tiles = (T + want - 1) / want;
    const dim3 grid((unsigned)((T + span_tiles - 1) / span_tiles), (unsigned)((n_slots + kTreeMomSlots - 1) / kTreeMomSlots));
    hipLaunchKernelGGL(tree_moments, grid, dim3(kTreeBlock), 0, st, q, slot, n_rows, span_tiles * kTreeTileRows, slot0,
                       n_slots, M);
    return (int)hipGetLastError();
}

int launch_tree_hist_reg(const uint8_t* bins, const uint32_t* q, const int32_t* slot, int64_t n_rows, const TreeGeom& gm,
                         int slot0, int n_slots, int64_t* hist, hipStream_t st) {
    unsigned long long* H = reinterpret_cast<unsigned long long*>(hist);
    const int64_t total = (int64_t)n_slots * gm.d * gm.bins * 2;
    hipLaunchKernelGGL(tree_zero, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 2048))),
                       dim3(256), 0, st, H, total);
    int e = (int)hipGetLastError();
    if (e || n_rows <= 0) return e;
    TreeGeom g = gm;
    g.n_sgroups = (n_slots + gm.sgroup - 1) / gm.sgroup;   // (a last group may be short)
    const int64_t items = g.n_spans * g.n_fchunks * g.n_sgroups;
    hipLaunchKernelGGL(tree_hist_reg, dim3((unsigned)items), dim3(kTreeBlock), (size_t)g.lds_bytes, st, bins, q, slot, n_rows,
                       g, slot0, n_slots, H);
    return (int)hipGetLastError();
}

int launch_tree_best_split_reg(const int64_t* hist, const int64_t* mom, const double* thr, const int32_t* nbins, int d,
                               int bins, int n_slots, int s, int64_t min_inst, double min_gain, double* rec, hipStream_t st) {
    hipLaunchKernelGGL(tree_best_split_reg, dim3((unsigned)n_slots), dim3(kTreeBlock), 0, st,
                       reinterpret_cast<const unsigned long long*>(hist), reinterpret_cast<const long long*>(mom), thr, nbins,
                       d, bins, s, (long long)min_inst, min_gain, rec);
    return (int)hipGetLastError();
}

}  // namespace psgd
