// psgd_metrics.hip -- binary classification metrics on the device (psgd_binary_counts*): from n
// (score, label) pairs the table of MLlib's BinaryClassificationMetrics with numBins = 0 -- one row
// {threshold, cumPos, cumNeg} per distinct score in descending java.lang.Double.compare order --
// and the two areas. A sort, a scan and a compaction; no streaming pass of the rows.
//
//   keys     score -> 64-bit key whose ascending order is the descending score order (negative
//            scores keep their bits, the others are complemented below the sign), label -> one
//            byte (label > 0.5); the 8 x 256 digit totals of all keys are counted on the way
//            (integer atomics), and metrics_plan marks the passes whose digit is the same in every
//            key: they are skipped on the device (the kernels of such a pass return at once), and
//            the plan tells every later kernel which of the two pair buffers holds its input.
//   sort     stable LSD radix sort of (key, byte) pairs, 8-bit digits, three plain launches a pass:
//            sort_hist (a tile's digit counts into the digit-major table), sort_scan (workgroup d
//            scans row d of the table, 256 tiles a sweep, from the total of the smaller digits),
//            sort_scatter (a tile's pairs ranked stably -- ballots over the digit's bits give a
//            lane its rank among the wave's equal digits, per-wave LDS counters order the waves
//            and the rounds -- gathered by digit in LDS and written out in runs).
//   groups   one three-phase scan over the sorted pairs carrying (group heads, positives): tile
//            sums, a scan of the tile sums by one workgroup (it also writes G, P, N), and the
//            tiles again: the last pair of each group writes its row of the table.
//   areas    rocNumerator = sum_g (cumNeg[g] - cumNeg[g-1]) (cumPos[g] + cumPos[g-1]) in 64-bit
//            integers (a workgroup's sum added with one integer atomic: exact in any order), the PR
//            trapezoids in fp64 per tile in a fixed order; areas_final adds the tiles' sums left to
//            right and divides the integer once.
//
// No workgroup waits on another: every dependency between workgroups is a kernel boundary (no
// look-back, no grid barrier, no cooperative launch). No floating-point atomics. Every element
// index is 64-bit; counts of at most n < 2^31 are 32-bit in the digit tables.
#include "psgd_internal.h"

namespace psgd {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kItems = 8;
constexpr int kTile = kBlock * kItems;   // pairs a workgroup sorts, scans or sums (metrics_tile())
constexpr int kDigits = 256;
constexpr int kPasses = 8;
constexpr uint64_t kSign = 0x8000000000000000ull;

__device__ __forceinline__ uint64_t key_of(double s) {
    const uint64_t b = (uint64_t)__double_as_longlong(s);
    return (b & kSign) ? b : (~b ^ kSign);
}
__device__ __forceinline__ double score_of(uint64_t k) {
    return __longlong_as_double((long long)((k & kSign) ? k : (~k ^ kSign)));
}

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}
// Inclusive scan of one value a thread over the workgroup, in thread order; total = the sum.
// sh holds kWaves entries and is free again when the call returns.
template <typename T>
__device__ __forceinline__ T block_incl_scan(T v, T* sh, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T s = wave_incl_scan(v, lane);
    if (lane == 63) sh[wave] = s;
    __syncthreads();
    T add = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const T x = sh[k];
        if (k < wave) add += x;
        tot += x;
    }
    total = tot;
    __syncthreads();
    return s + add;
}

// ---- keys ----
__global__ __launch_bounds__(kBlock) void metrics_keys(const double* __restrict__ scores,
                                                       const double* __restrict__ labels, int64_t n,
                                                       uint64_t* __restrict__ keys, uint8_t* __restrict__ bytes,
                                                       unsigned* __restrict__ ghist) {
    __shared__ unsigned hist[kPasses * kDigits];
    for (int i = threadIdx.x; i < kPasses * kDigits; i += kBlock) hist[i] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const uint64_t k = key_of(scores[i]);
        keys[i] = k;
        bytes[i] = labels[i] > 0.5 ? 1 : 0;
#pragma unroll
        for (int p = 0; p < kPasses; ++p) atomicAdd(&hist[p * kDigits + (int)((k >> (8 * p)) & 255)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kPasses * kDigits; i += kBlock) {
        const unsigned c = hist[i];
        if (c) atomicAdd(&ghist[i], c);
    }
}

// plan[p] (p < 8): the pair buffer pass p reads (0 / 1), or -1 when every key has the same digit p
// (the pass is skipped); plan[8]: the buffer that holds the sorted pairs.
__global__ __launch_bounds__(kBlock) void metrics_plan(const unsigned* __restrict__ ghist, int64_t n,
                                                       int* __restrict__ plan) {
    __shared__ int constant[kPasses];
    if (threadIdx.x < kPasses) constant[threadIdx.x] = 0;
    __syncthreads();
    for (int p = 0; p < kPasses; ++p)
        if ((int64_t)ghist[p * kDigits + threadIdx.x] == n) constant[p] = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        int cur = 0;
        for (int p = 0; p < kPasses; ++p) {
            if (constant[p]) {
                plan[p] = -1;
            } else {
                plan[p] = cur;
                cur ^= 1;
            }
        }
        plan[kPasses] = cur;
    }
}

struct Pairs {
    uint64_t* keys[2];
    uint8_t* bytes[2];
};

// ---- sort ----
__global__ __launch_bounds__(kBlock) void sort_hist(Pairs B, const int* __restrict__ plan, int pass, int64_t n,
                                                    int64_t n_tiles, unsigned* __restrict__ table) {
    const int src = plan[pass];
    if (src < 0) return;
    __shared__ unsigned hist[kDigits];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t* keys = B.keys[src];
    const int64_t base = (int64_t)blockIdx.x * kTile;
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int64_t i = base + r * kBlock + threadIdx.x;
        if (i < n) atomicAdd(&hist[(int)((keys[i] >> (8 * pass)) & 255)], 1u);
    }
    __syncthreads();
    table[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = hist[threadIdx.x];
}

// Workgroup d: row d of the digit-major table becomes each tile's first output index for digit d.
__global__ __launch_bounds__(kBlock) void sort_scan(const int* __restrict__ plan, int pass,
                                                    const unsigned* __restrict__ ghist, int64_t n_tiles,
                                                    unsigned* __restrict__ table) {
    if (plan[pass] < 0) return;
    __shared__ unsigned sh[kWaves];
    const int d = blockIdx.x;
    unsigned carry;
    (void)block_incl_scan<unsigned>((int)threadIdx.x < d ? ghist[pass * kDigits + threadIdx.x] : 0u, sh, carry);
    unsigned* row = table + (int64_t)d * n_tiles;
    for (int64_t c = 0; c < n_tiles; c += kBlock) {
        const int64_t t = c + threadIdx.x;
        const unsigned v = t < n_tiles ? row[t] : 0u;
        unsigned total;
        const unsigned incl = block_incl_scan<unsigned>(v, sh, total);
        if (t < n_tiles) row[t] = carry + incl - v;
        carry += total;
    }
}

// The lanes of the wave whose element is valid and has this lane's digit.
__device__ __forceinline__ uint64_t match_digit(unsigned digit, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

__global__ __launch_bounds__(kBlock) void sort_scatter(Pairs B, const int* __restrict__ plan, int pass, int64_t n,
                                                       int64_t n_tiles, const unsigned* __restrict__ table) {
    const int src = plan[pass];
    if (src < 0) return;
    __shared__ uint64_t keys_l[kTile];
    __shared__ uint8_t bytes_l[kTile];
    __shared__ unsigned hist[kDigits];
    __shared__ unsigned run[kDigits];          // the next local slot of a digit
    __shared__ long long gdelta[kDigits];      // a digit's output index minus its local slot
    __shared__ unsigned wave_cnt[kWaves][kDigits];
    __shared__ unsigned sh[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t* keys = B.keys[src];
    const uint8_t* bytes = B.bytes[src];
    uint64_t* out_keys = B.keys[src ^ 1];
    uint8_t* out_bytes = B.bytes[src ^ 1];
    const int64_t base = (int64_t)blockIdx.x * kTile;
    const int count = (int)(n - base < kTile ? n - base : kTile);
    const int shift = 8 * pass;

    uint64_t k[kItems];
    uint8_t b[kItems];
    hist[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int il = r * kBlock + threadIdx.x;
        k[r] = 0;
        b[r] = 0;
        if (il < count) {
            k[r] = keys[base + il];
            b[r] = bytes[base + il];
            atomicAdd(&hist[(int)((k[r] >> shift) & 255)], 1u);
        }
    }
    __syncthreads();
    {
        const unsigned c = hist[threadIdx.x];
        unsigned total;
        const unsigned excl = block_incl_scan<unsigned>(c, sh, total) - c;
        run[threadIdx.x] = excl;
        gdelta[threadIdx.x] = (long long)table[(int64_t)threadIdx.x * n_tiles + blockIdx.x] - (long long)excl;
    }
    __syncthreads();
    // the tile's elements in index order are rounds of 256, a round's in wave order, a wave's in
    // lane order: a digit's slots are handed out in that order
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
#pragma unroll
        for (int w = 0; w < kWaves; ++w) wave_cnt[w][threadIdx.x] = 0;
        __syncthreads();
        const bool valid = r * kBlock + (int)threadIdx.x < count;
        const unsigned digit = (unsigned)((k[r] >> shift) & 255);
        const uint64_t m = match_digit(digit, valid);
        const unsigned rank = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wave_cnt[wave][digit] = (unsigned)__popcll(m);
        __syncthreads();
        {
            unsigned o = run[threadIdx.x];
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const unsigned c = wave_cnt[w][threadIdx.x];
                wave_cnt[w][threadIdx.x] = o;
                o += c;
            }
            run[threadIdx.x] = o;
        }
        __syncthreads();
        if (valid) {
            const unsigned pos = wave_cnt[wave][digit] + rank;
            if (pos < (unsigned)kTile) {
                keys_l[pos] = k[r];
                bytes_l[pos] = b[r];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int il = r * kBlock + threadIdx.x;
        if (il < count) {
            const uint64_t key = keys_l[il];
            const long long dst = gdelta[(int)((key >> shift) & 255)] + il;
            if (dst >= 0 && dst < n) {
                out_keys[dst] = key;
                out_bytes[dst] = bytes_l[il];
            }
        }
    }
}

// ---- groups ----
// Thread t of a tile takes its pairs t * 8 .. t * 8 + 7 in order. head: the first pair of a group.
__device__ __forceinline__ void load_flags(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ bytes,
                                           int64_t i0, int64_t n, uint64_t k[kItems], unsigned& heads,
                                           unsigned& pos, unsigned& head_bits, unsigned& pos_bits) {
    uint64_t prev = i0 > 0 && i0 - 1 < n ? keys[i0 - 1] : 0;
    heads = pos = 0;
    head_bits = pos_bits = 0;
    uint8_t b[kItems];
    if (i0 + kItems <= n) {   // a whole run: unguarded, so that the loads are wide
#pragma unroll
        for (int e = 0; e < kItems; ++e) {
            k[e] = keys[i0 + e];
            b[e] = bytes[i0 + e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < kItems; ++e) {
            k[e] = i0 + e < n ? keys[i0 + e] : 0;
            b[e] = i0 + e < n ? bytes[i0 + e] : 0;
        }
    }
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
        const int64_t i = i0 + e;
        if (i < n) {
            const bool h = i == 0 || k[e] != prev;
            const bool p = b[e] != 0;
            heads += h;
            pos += p;
            head_bits |= (unsigned)h << e;
            pos_bits |= (unsigned)p << e;
            prev = k[e];
        }
    }
}

__global__ __launch_bounds__(kBlock) void groups_reduce(Pairs B, const int* __restrict__ plan, int64_t n,
                                                        long long* __restrict__ tile_heads,
                                                        long long* __restrict__ tile_pos) {
    const int src = plan[kPasses];
    __shared__ unsigned sh[kWaves];
    uint64_t k[kItems];
    unsigned heads, pos, hb, pb;
    load_flags(B.keys[src], B.bytes[src], (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems, n, k, heads,
               pos, hb, pb);
    unsigned th, tp;
    (void)block_incl_scan<unsigned>(heads, sh, th);
    (void)block_incl_scan<unsigned>(pos, sh, tp);
    if (threadIdx.x == 0) {
        tile_heads[blockIdx.x] = th;
        tile_pos[blockIdx.x] = tp;
    }
}

// One workgroup: the tiles' sums become the sums of the tiles before them; summary = {G, P, N, 0}.
__global__ __launch_bounds__(kBlock) void groups_scan_tiles(int64_t n, int64_t n_tiles,
                                                            long long* __restrict__ tile_heads,
                                                            long long* __restrict__ tile_pos,
                                                            long long* __restrict__ summary) {
    __shared__ long long sh[kWaves];
    long long ch = 0, cp = 0;
    for (int64_t c = 0; c < n_tiles; c += kBlock) {
        const int64_t t = c + threadIdx.x;
        const long long h = t < n_tiles ? tile_heads[t] : 0, p = t < n_tiles ? tile_pos[t] : 0;
        long long th, tp;
        const long long ih = block_incl_scan<long long>(h, sh, th);
        const long long ip = block_incl_scan<long long>(p, sh, tp);
        if (t < n_tiles) {
            tile_heads[t] = ch + ih - h;
            tile_pos[t] = cp + ip - p;
        }
        ch += th;
        cp += tp;
    }
    if (threadIdx.x == 0) {
        summary[0] = ch;
        summary[1] = cp;
        summary[2] = n - cp;
        summary[3] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void groups_write(Pairs B, const int* __restrict__ plan, int64_t n,
                                                       const long long* __restrict__ tile_heads,
                                                       const long long* __restrict__ tile_pos,
                                                       double* __restrict__ thresholds,
                                                       long long* __restrict__ cum_pos,
                                                       long long* __restrict__ cum_neg) {
    const int src = plan[kPasses];
    __shared__ unsigned sh[kWaves];
    const uint64_t* keys = B.keys[src];
    const int64_t i0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
    uint64_t k[kItems];
    unsigned heads, pos, hb, pb;
    load_flags(keys, B.bytes[src], i0, n, k, heads, pos, hb, pb);
    unsigned th, tp;
    long long H = tile_heads[blockIdx.x] + (block_incl_scan<unsigned>(heads, sh, th) - heads);
    long long Pc = tile_pos[blockIdx.x] + (block_incl_scan<unsigned>(pos, sh, tp) - pos);
    // the key after this thread's last pair
    const int64_t after = i0 + kItems;
    const uint64_t next_key = after < n ? keys[after] : 0;
#pragma unroll
    for (int e = 0; e < kItems; ++e) {
        const int64_t i = i0 + e;
        if (i >= n) break;
        H += (hb >> e) & 1u;
        Pc += (pb >> e) & 1u;
        const bool last = i == n - 1 || (e + 1 < kItems ? k[e + 1] : next_key) != k[e];
        if (last) {
            const long long g = H - 1;
            if (g >= 0 && g < n) {
                if (thresholds) thresholds[g] = score_of(k[e]);
                cum_pos[g] = Pc;
                cum_neg[g] = (i + 1) - Pc;
            }
        }
    }
}

// ---- areas ----
__device__ __forceinline__ double readlane_f64(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), l);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__global__ __launch_bounds__(kBlock) void areas_tiles(const long long* __restrict__ cum_pos,
                                                      const long long* __restrict__ cum_neg,
                                                      long long* __restrict__ summary,
                                                      double* __restrict__ tile_pr) {
    __shared__ double pr_sh[kWaves];
    __shared__ unsigned long long roc_sh[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long G = summary[0], P = summary[1];
    const int64_t g0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kItems;
    double pr = 0.0;
    unsigned long long roc = 0;
    if (g0 < G) {
        long long pp = 0, pn = 0;
        double rec_prev = 0.0, prec_prev = 1.0;
        if (g0 > 0) {
            pp = cum_pos[g0 - 1];
            pn = cum_neg[g0 - 1];
            rec_prev = P ? (double)pp / (double)P : 0.0;
            prec_prev = (double)pp / (double)(pp + pn);
        }
        long long cps[kItems], cns[kItems];
        if (g0 + kItems <= G) {   // a whole run: unguarded, so that the loads are wide
#pragma unroll
            for (int e = 0; e < kItems; ++e) {
                cps[e] = cum_pos[g0 + e];
                cns[e] = cum_neg[g0 + e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < kItems; ++e) {
                cps[e] = g0 + e < G ? cum_pos[g0 + e] : 0;
                cns[e] = g0 + e < G ? cum_neg[g0 + e] : 0;
            }
        }
#pragma unroll
        for (int e = 0; e < kItems; ++e) {
            const int64_t g = g0 + e;
            if (g >= G) break;
            const long long cp = cps[e], cn = cns[e];
            const double rec = P ? (double)cp / (double)P : 0.0;
            const double prec = (double)cp / (double)(cp + cn);
            pr = pr + (rec - rec_prev) * (prec + prec_prev) / 2.0;
            roc += (unsigned long long)(cn - pn) * (unsigned long long)(cp + pp);
            pp = cp;
            pn = cn;
            rec_prev = rec;
            prec_prev = prec;
        }
    }
    // the threads' sums in a fixed tree: a butterfly over the lanes, then the waves in order
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        pr = pr + __shfl_xor(pr, m, 64);
        roc += __shfl_xor(roc, m, 64);
    }
    if (lane == 0) {
        pr_sh[wave] = pr;
        roc_sh[wave] = roc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = pr_sh[0];
        unsigned long long r = roc_sh[0];
        for (int w = 1; w < kWaves; ++w) {
            s = s + pr_sh[w];
            r += roc_sh[w];
        }
        tile_pr[blockIdx.x] = s;
        if (r) atomicAdd(reinterpret_cast<unsigned long long*>(summary + 3), r);
    }
}

// One wave: the tiles' PR sums added left to right; the ROC integer divided once.
__global__ __launch_bounds__(64) void areas_final(const long long* __restrict__ summary,
                                                  const double* __restrict__ tile_pr, double* __restrict__ areas) {
    const int lane = threadIdx.x;
    const long long G = summary[0], P = summary[1], N = summary[2], num = summary[3];
    const int64_t nt = (G + kTile - 1) / kTile;
    // 64 sums a load (the next 64 in flight meanwhile), added in lane order: one dependent add a tile
    double s = 0.0;
    double x = lane < nt ? tile_pr[lane] : 0.0;
    int64_t b = 0;
    for (; b + 64 <= nt; b += 64) {
        const double nx = b + 64 + lane < nt ? tile_pr[b + 64 + lane] : 0.0;
#pragma unroll
        for (int q = 0; q < 64; ++q) s = s + readlane_f64(x, q);
        x = nx;
    }
    const int m = (int)(nt - b);
    for (int q = 0; q < m; ++q) s = s + readlane_f64(x, q);
    if (lane == 0) {
        areas[0] = P == 0 ? 0.0 : N == 0 ? 1.0 : (double)num / (2.0 * (double)P * (double)N);
        areas[1] = s;
    }
}

}  // namespace

int32_t metrics_tile() { return kTile; }

int launch_metrics_begin(const MetricsBufs& B, hipStream_t st) {
    return (int)hipMemsetAsync(B.ghist, 0, kPasses * kDigits * sizeof(unsigned), st);
}

int launch_metrics_keys(const MetricsBufs& B, const double* scores, const double* labels, int64_t offset,
                        int64_t n, int num_cus, hipStream_t st) {
    if (n <= 0) return 0;
    const int64_t want = (n + kTile - 1) / kTile;
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 8;
    hipLaunchKernelGGL(metrics_keys, dim3((unsigned)(want < cap ? want : cap)), dim3(kBlock), 0, st, scores, labels,
                       n, B.keys[0] + offset, B.bytes[0] + offset, B.ghist);
    return (int)hipGetLastError();
}

int launch_metrics_finish(const MetricsBufs& B, int64_t n, double* thresholds, int64_t* cum_pos, int64_t* cum_neg,
                          int64_t* summary, double* areas, hipStream_t st) {
    if (n <= 0 || n > (int64_t)INT32_MAX) return (int)hipErrorInvalidValue;
    const int64_t n_tiles = (n + kTile - 1) / kTile;
    const dim3 tiles((unsigned)n_tiles), block(kBlock);
    Pairs pr;
    pr.keys[0] = B.keys[0];
    pr.keys[1] = B.keys[1];
    pr.bytes[0] = B.bytes[0];
    pr.bytes[1] = B.bytes[1];
    hipLaunchKernelGGL(metrics_plan, dim3(1), block, 0, st, B.ghist, n, B.plan);
    for (int pass = 0; pass < kPasses; ++pass) {
        hipLaunchKernelGGL(sort_hist, tiles, block, 0, st, pr, B.plan, pass, n, n_tiles, B.table);
        hipLaunchKernelGGL(sort_scan, dim3(kDigits), block, 0, st, B.plan, pass, B.ghist, n_tiles, B.table);
        hipLaunchKernelGGL(sort_scatter, tiles, block, 0, st, pr, B.plan, pass, n, n_tiles, B.table);
    }
    long long* th = reinterpret_cast<long long*>(B.tile_heads);
    long long* tp = reinterpret_cast<long long*>(B.tile_pos);
    long long* cp = reinterpret_cast<long long*>(cum_pos);
    long long* cn = reinterpret_cast<long long*>(cum_neg);
    long long* sm = reinterpret_cast<long long*>(summary);
    hipLaunchKernelGGL(groups_reduce, tiles, block, 0, st, pr, B.plan, n, th, tp);
    hipLaunchKernelGGL(groups_scan_tiles, dim3(1), block, 0, st, n, n_tiles, th, tp, sm);
    hipLaunchKernelGGL(groups_write, tiles, block, 0, st, pr, B.plan, n, th, tp, thresholds, cp, cn);
    hipLaunchKernelGGL(areas_tiles, tiles, block, 0, st, cp, cn, sm, B.tile_pr);
    hipLaunchKernelGGL(areas_final, dim3(1), dim3(64), 0, st, sm, B.tile_pr, areas);
    return (int)hipGetLastError();
}

}  // namespace psgd
