// psgd_kmeans.hip -- Lloyd's iteration of k-means over the registered partitions (psgd_kmeans_assign,
// psgd_kmeans_step, psgd_kmeans_update_device). Centres C are k x d doubles, row-major, k <= 256. All
// arithmetic is fp64 whatever the storage. For a row x: g_j = x . c_j (one fma chain along the
// features), cn_j = ||c_j||^2 (one chain, once a call), s_j = fma(-2, g_j, cn_j); the assignment is the
// smallest j that minimises s_j (strict <, ties to the lowest index); xn = ||x||^2;
// dist2 = max(xn + s_a, 0). A step returns {sums[k][d], counts[k], cost, n}: the rows summed by
// centre, the rows counted by centre, the sum of dist2, the row count.
//
// Rows are cut into tiles of gm.tile_rows rows numbered across the partitions in partition-index order
// (KmPart::tile0), so one launch serves every partition; KmPart::row0 places a partition in the local
// row order of assign / dist2.
//
// kmeans_pack_c writes C^T (d x k) into project_pack_b's operand order (index ((s nb + b) VEC + e) 64
// + l holds C[16 b + (l & 15)][(4 s + (l >> 4)) VEC + e], zero past d or k) and cn [kpad], with +Inf at
// the pad centres; the argmin masks them by selection as well.
//
// Dense rows, assignment: v_mfma_f64_16x16x4_f64 with M = rows, K = features, N = centres, in
// project_dense's geometry. An item is a 16-row tile: the wave walks the chunks of CB centre blocks
// itself (from the second chunk on its 16 rows come from L2). Lane l = (m = l & 15, q = l >> 4) reads
// row m as 16-byte vectors at the row's own pitch; loads carry no branch, a vector past the row's last
// reloads the last, a row past the tile's end the partition's last row, a feature >= d is replaced by
// 0.0 by selection. After a chunk the lane holds D[row = q + 4 reg][centre = 16 b + m]; it folds its
// blocks into a running (min, index) per row in ascending block order with strict <. When the chunks
// are done, the 16 lanes of a DPP row reduce their (value, index) pairs, the lower index winning an
// equal value. ||x||^2 is accumulated from the lane's own A operands in the first chunk's walk, reduced
// over the four q lanes of a row in a fixed order, and meets the row's minimum in lane m + 16 (m & 3),
// which writes assign and dist2. A tile's sum of dist2 is added in row order into one record; the
// records are merged in tile order (grad_merge_records). No atomics; the same bits from call to call.
//
// Dense rows, sums: the same instruction with M = centres, N = features, K = rows: gram_dense with the
// A operand replaced. For rows i0 .. i0 + 3 the B operand is the fragment z[i0 + (l >> 4)][16 fb + (l &
// 15)] of the rows as they lie, with 1.0 at column d (the counts); the A operand is A[m][q] =
// (assign[i0 + q] == 16 cb + m) ? 1.0 : 0.0, by selection. A wave keeps gr x gc blocks (centre blocks x
// feature blocks; 4 x 8 = 256 accumulator registers at most) over a span of tiles; an item is (span,
// rectangle), span-major, and ends with one record; kmeans_merge adds the records in span order. The
// products are 1.0 x or 0.0 x, exact, so a sum is a fixed-order fp64 chain over the member rows: no
// floating-point atomics, the same bits from call to call, nothing depends on the grid. A column >= d
// loads feature d - 1 instead: a zero-copy row's pad is never read.
//
// CSR rows, assignment: project_csr's design. A group of gl lanes (the power of two >= k, at most 64)
// takes a row, lane j keeps centres j, j + gl, .. (four at most), g_j accumulated with fma in entry
// order, C^T's rows from LDS while d x kpad doubles fit, else the caller's C through L2; xn in entry
// order; the argmin over the group with the same tie rule. No atomics; the same bits from call to call.
//
// CSR rows, sums: one fp64 atomic add an entry into sums[a][col], into LDS accumulators while k d <=
// 6,144 doubles (flushed with one global atomic a non-zero accumulator), else into global memory; the
// counts with integer atomics, exact. assign, dist2, cost and counts repeat bit for bit; the CSR sums
// repeat only up to their last bits (the atomics' order), as for gram_csr.
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

#include <algorithm>

#include "psgd_device.h"

namespace psgd {
namespace {

constexpr int kKmBlock = 512;               // the assign kernels
constexpr int kKmWaves = kKmBlock / 64;
constexpr int kKmU = 4;                     // steps whose vectors are loaded together (one stage)
constexpr int64_t kKmLds = 160 * 1024;      // a CU's LDS
constexpr int kKmCsrTile = 256;             // CSR rows a tile
constexpr int kKmSumBlock = 256;            // the sums kernels
constexpr int kKmSumWaves = kKmSumBlock / 64;
constexpr int kKmSub = 2;                   // 4-row steps whose fragments are loaded together (one stage)
constexpr int64_t kKmItems = 2048;          // items the sums' plan aims at
constexpr int kKmLdsSums = 6144;            // CSR sums: fp64 accumulators a workgroup keeps in LDS
typedef double km_d4 __attribute__((ext_vector_type(4)));

// The tile's partition: the last p with tab[p].tile0 <= tile. Uniform over the wave.
__device__ __forceinline__ int km_partition(const KmPart* tab, int P, int64_t tile) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void kmeans_zero(double* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0.0;
}

// total = dpad kpad operands of Cp (0: CSR rows, cn alone); block 0 writes cn [16 nb].
__global__ __launch_bounds__(256) void kmeans_pack_c(const double* __restrict__ C, int d, int k, int nb, int vec,
                                                     int64_t total, double* __restrict__ Cp, double* __restrict__ cn) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int l = (int)(i & 63);
        int64_t t = i >> 6;
        const int e = (int)(t % vec);
        t /= vec;
        const int b = (int)(t % nb);
        const int64_t s = t / nb;
        const int64_t f = (4 * s + (l >> 4)) * vec + e;
        const int c = 16 * b + (l & 15);
        Cp[i] = f < d && c < k ? C[(int64_t)c * d + f] : 0.0;
    }
    const int j = threadIdx.x;
    if (blockIdx.x == 0 && j < 16 * nb) {
        double s = __builtin_inf();
        if (j < k) {
            s = 0.0;
            for (int f = 0; f < d; ++f) {
                const double c = C[(int64_t)j * d + f];
                s = m_fma(c, c, s);
            }
        }
        cn[j] = s;
    }
}

// One butterfly step of the (value, index) argmin over a DPP row: the partner's pair wins when its
// value is smaller, or equal at a lower index. Both partners end with the same pair.
template <int CTRL>
__device__ __forceinline__ void km_argmin_step(double& v, int& i) {
    const double pv = dpp_mov<CTRL>(v);
    const int pi = __builtin_amdgcn_mov_dpp(i, CTRL, 0xF, 0xF, true);
    const bool take = pv < v || (pv == v && pi < i);
    v = take ? pv : v;
    i = take ? pi : i;
}

template <typename S, int CB, bool LDSB>
__global__ __launch_bounds__(kKmBlock) void kmeans_assign_dense(const ChainDesc* __restrict__ descs,
                                                                const KmPart* __restrict__ tab, int P, int64_t n_tiles,
                                                                KmGeom gm, const double* __restrict__ Cp,
                                                                const double* __restrict__ cn,
                                                                int32_t* __restrict__ assign, double* __restrict__ dist2,
                                                                double* __restrict__ rec) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    extern __shared__ double km_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = gm.d, k = gm.k, nb = gm.nb;
    const int nsteps = gm.dpad / (4 * VEC);
    if constexpr (LDSB) {
        const int total = gm.dpad * gm.kpad;   // a multiple of 128
        for (int i = 2 * (int)threadIdx.x; i < total; i += 2 * kKmBlock) {
            const f64x2 v = *reinterpret_cast<const f64x2*>(Cp + i);
            *reinterpret_cast<f64x2*>(km_lds + i) = v;
        }
        __syncthreads();
    }
    const int m = lane & 15, q = lane >> 4;
    const int nvec = (d + VEC - 1) / VEC;       // the row's vectors that hold a feature (<= ld / VEC)
    const int nchunk = (nb + CB - 1) / CB;
    const double inf = __builtin_inf();
    for (int64_t tile = (int64_t)blockIdx.x * kKmWaves + wave; tile < n_tiles; tile += (int64_t)gridDim.x * kKmWaves) {
        const int p = km_partition(tab, P, tile);
        const KmPart pp = tab[p];
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - pp.tile0) * 16;
        if (r0 >= dsc.n_rows) {   // (no tile is cut past a partition's end)
            if (lane == 0) rec[tile] = 0.0;
            continue;
        }
        const int64_t row = r0 + m;
        const int64_t rr = row < dsc.n_rows ? row : dsc.n_rows - 1;
        const gptr<V> xr = as_global(reinterpret_cast<const V*>(reinterpret_cast<const S*>(dsc.x) + rr * dsc.ld));
        // the running minimum of rows q, q + 4, q + 8, q + 12 over this lane's centres, and the lane's
        // share of ||x_m||^2
        double bv[4] = {inf, inf, inf, inf};
        int bix[4] = {0, 0, 0, 0};
        double xn = 0.0;

        // A stage's loads carry no branch: a vector past the row's last loads the last (in bounds at
        // the row's own pitch), and what it holds at a feature >= d is replaced at its use.
        auto load = [&](V (&xv)[kKmU], int s0) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < kKmU; ++u) {
                const int vi = 4 * (s0 + u) + q;
                xv[u] = xr[vi < nvec ? vi : nvec - 1];
            }
        };
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            // the chunk's blocks; one past the last repeats the last and is not used
            int bi[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c) bi[c] = chunk * CB + c < nb ? chunk * CB + c : nb - 1;
            km_d4 acc[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c) acc[c] = km_d4{0.0, 0.0, 0.0, 0.0};
            const bool first = chunk == 0;   // (uniform)
            auto compute = [&](const V (&xv)[kKmU], int s0) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < kKmU; ++u) {
                    const int s = s0 + u;
                    if (s >= nsteps) break;   // (uniform)
                    double a[VEC];
                    unpack<S, double>(xv[u], a);
                    const int f0 = (4 * s + q) * VEC;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) a[e] = f0 + e < d ? a[e] : 0.0;
                    if (first) {
#pragma unroll
                        for (int e = 0; e < VEC; ++e) xn = m_fma(a[e], a[e], xn);
                    }
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
#pragma unroll
                        for (int c = 0; c < CB; ++c) {
                            double b;
                            if constexpr (LDSB)
                                b = km_lds[((s * nb + bi[c]) * VEC + e) * 64 + lane];
                            else
                                b = as_global(Cp)[(((int64_t)s * nb + bi[c]) * VEC + e) * 64 + lane];
                            acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], b, acc[c], 0, 0, 0);
                        }
                }
            };
            // two sets of vectors: the next stage's loads are in flight under this stage's MFMAs
            V xa[kKmU], xb[kKmU];
            int s0 = 0;
            load(xa, 0);
            while (s0 < nsteps) {
                load(xb, s0 + kKmU);
                compute(xa, s0);
                s0 += kKmU;
                if (s0 >= nsteps) break;
                load(xa, s0 + kKmU);
                compute(xb, s0);
                s0 += kKmU;
            }
            // D[q + 4 g][16 blk + m]: the lane's centre of each block against four rows, ascending blocks
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                const int blk = chunk * CB + c;
                if (blk >= nb) break;   // (uniform)
                const int centre = blk * 16 + m;
                const double cnv = as_global(cn)[centre];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const double s = centre < k ? m_fma(-2.0, acc[c][g], cnv) : inf;
                    const bool take = s < bv[g];
                    bv[g] = take ? s : bv[g];
                    bix[g] = take ? centre : bix[g];
                }
            }
        }
        // over the 16 lanes of the DPP row: every lane of row q ends with rows q + 4 g's pairs
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            km_argmin_step<0xB1>(bv[g], bix[g]);    // quad_perm [1,0,3,2]
            km_argmin_step<0x4E>(bv[g], bix[g]);    // quad_perm [2,3,0,1]
            km_argmin_step<0x141>(bv[g], bix[g]);   // row_half_mirror
            km_argmin_step<0x140>(bv[g], bix[g]);   // row_mirror
        }
        // ||x_m||^2 over the four q lanes of row m: (q0 + q1) + (q2 + q3), the same in all four
        xn = swap_sum32(swap_sum16(xn));
        // row m = q + 4 g meets its minimum in the lane with q = m & 3
        const int g = m >> 2;
        const double sv = g == 0 ? bv[0] : g == 1 ? bv[1] : g == 2 ? bv[2] : bv[3];
        const int si = g == 0 ? bix[0] : g == 1 ? bix[1] : g == 2 ? bix[2] : bix[3];
        const bool writer = (m & 3) == q && row < dsc.n_rows;
        double d2 = xn + sv;
        d2 = d2 > 0.0 ? d2 : 0.0;
        d2 = writer ? d2 : 0.0;
        if (writer) {
            assign[pp.row0 + row] = si;
            if (dist2) dist2[pp.row0 + row] = d2;
        }
        // the tile's cost in row order (rows past the end add 0.0)
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += readlane_d(d2, r + 16 * (r & 3));
        if (lane == 0) rec[tile] = t;
    }
}

template <typename S, int GR, int GC>
__global__ __launch_bounds__(kKmSumBlock, 1) void kmeans_sums_dense(const ChainDesc* __restrict__ descs,
                                                                   const KmPart* __restrict__ tab, int P,
                                                                   int64_t n_tiles, KmGeom gm,
                                                                   const int32_t* __restrict__ assign,
                                                                   double* __restrict__ rec) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t item = (int64_t)blockIdx.x * kKmSumWaves + wave;
    if (item >= gm.n_items) return;
    const int n_rects = gm.nrg * gm.ncg;
    const int64_t span = item / n_rects;
    const int rect = (int)(item - span * n_rects);
    const int R = rect / gm.ncg, C = rect - R * gm.ncg;
    const int jb0 = R * GR, kb0 = C * GC;
    const int d = gm.d;
    // block (r, c) of the rectangle is computed when it lies inside [centres] x [features, 1]
    unsigned on = 0;
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c)
            if (jb0 + r < gm.nb && kb0 + c < gm.nbf) on |= 1u << (r * GC + c);
    on = __builtin_amdgcn_readfirstlane(on);
    const int m = lane & 15, kq = lane >> 4;
    // the lane's centre of each A fragment; its column of each B fragment and the feature it loads (a
    // column >= d loads feature d - 1, in bounds and never a pad column; its value is not used)
    int cen[GR], cb[GC], lb[GC];
#pragma unroll
    for (int r = 0; r < GR; ++r) cen[r] = (jb0 + r) * 16 + m;
#pragma unroll
    for (int c = 0; c < GC; ++c) {
        cb[c] = (kb0 + c) * 16 + m;
        lb[c] = cb[c] < d ? cb[c] : d - 1;
    }
    km_d4 acc[GR][GC];
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c) acc[r][c] = km_d4{0.0, 0.0, 0.0, 0.0};

    const int64_t t0 = span * gm.span;
    const int64_t t1 = t0 + gm.span < n_tiles ? t0 + gm.span : n_tiles;
    // the span's tiles, a partition's run of them at a time: consecutive tiles of a partition are
    // consecutive rows, walked four rows a step
    int64_t tile = t0;
    while (tile < t1) {
        const int p = km_partition(tab, P, tile);
        const KmPart pp = tab[p];
        const ChainDesc dsc = descs[p];
        const int64_t pe = tab[p + 1].tile0;   // (> tile: p is the last partition that starts at or before it)
        const int64_t te = pe < t1 ? pe : t1;
        const int64_t r0 = (tile - pp.tile0) * 16;
        const int64_t re = (te - pp.tile0) * 16;
        const int64_t r1 = re < dsc.n_rows ? re : dsc.n_rows;
        tile = te;
        if (r1 <= r0) continue;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        const int32_t* arow = assign + pp.row0;
        // A stage's loads carry no branch and no conversion: a row past the run's end loads its last
        // row, and the selection at the use keeps it out of the sums.
        auto load = [&](S (&fb)[kKmSub][GC], int (&fa)[kKmSub], int64_t rb) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < kKmSub; ++s) {
                const int64_t row = rb + 4 * s + kq;
                const int64_t rr = row < r1 ? row : r1 - 1;
                const gptr<S> xr = as_global(X + rr * dsc.ld);
#pragma unroll
                for (int c = 0; c < GC; ++c) fb[s][c] = xr[lb[c]];
                fa[s] = as_global(arow)[rr];
            }
        };
        auto compute = [&](const S (&fb)[kKmSub][GC], const int (&fa)[kKmSub], int64_t rb) __attribute__((always_inline)) {
            unsigned onl = __builtin_amdgcn_readfirstlane(on);
            asm volatile("" : "+s"(onl));
#pragma unroll
            for (int s = 0; s < kKmSub; ++s) {
                const bool valid = rb + 4 * s + kq < r1;
                double a[GR], b[GC];
#pragma unroll
                for (int r = 0; r < GR; ++r) a[r] = valid && fa[s] == cen[r] ? 1.0 : 0.0;
#pragma unroll
                for (int c = 0; c < GC; ++c) b[c] = cb[c] < d ? (double)fb[s][c] : cb[c] == d ? 1.0 : 0.0;
#pragma unroll
                for (int r = 0; r < GR; ++r)
#pragma unroll
                    for (int c = 0; c < GC; ++c)
                        if ((onl >> (r * GC + c)) & 1u)
                            acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[c], acc[r][c], 0, 0, 0);
            }
        };
        // two sets of fragments: the next stage's loads are in flight under this stage's MFMAs
        constexpr int64_t stage = 4 * kKmSub;
        S xa[kKmSub][GC], xb[kKmSub][GC];
        int aa[kKmSub], ab[kKmSub];
        int64_t rb = r0;
        load(xa, aa, rb);
        while (rb < r1) {
            load(xb, ab, rb + stage);
            compute(xa, aa, rb);
            rb += stage;
            if (rb >= r1) break;
            load(xa, aa, rb + stage);
            compute(xb, ab, rb);
            rb += stage;
        }
    }
    // block (r, c)'s 256 doubles lie row-major: reg * 64 + lane = 16 * ((lane >> 4) + 4 reg) + (lane & 15)
    double* out = rec + item * ((int64_t)GR * GC * 256);
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c)
            if ((on >> (r * GC + c)) & 1u) {
#pragma unroll
                for (int g = 0; g < 4; ++g) out[((r * GC + c) * 4 + g) * 64 + lane] = acc[r][c][g];
            }
}

// Thread (centre j, column f <= d): the spans' records added in span order. Column d is the count.
__global__ __launch_bounds__(kKmSumBlock) void kmeans_merge(const double* __restrict__ rec, KmGeom gm,
                                                            double* __restrict__ out) {
    const int f = blockIdx.x * kKmSumBlock + threadIdx.x;
    const int j = blockIdx.y;
    if (f > gm.d || j >= gm.k) return;
    const int jb = j >> 4, fb = f >> 4;
    const int R = jb / gm.gr, C = fb / gm.gc;
    const int64_t recsz = (int64_t)gm.gr * gm.gc * 256;
    const int64_t n_rects = (int64_t)gm.nrg * gm.ncg;
    const double* src = rec + (R * gm.ncg + C) * recsz + (int64_t)((jb - R * gm.gr) * gm.gc + (fb - C * gm.gc)) * 256 +
                        (j & 15) * 16 + (f & 15);
    double s = 0.0;
    for (int64_t sp = 0; sp < gm.n_spans; ++sp) s += src[sp * n_rects * recsz];
    if (f < gm.d) out[(int64_t)j * gm.d + f] = s;
    else out[(int64_t)gm.k * gm.d + j] = s;
}

// out's tail: the counts (CSR: from the integer accumulators), the cost, the row count.
__global__ __launch_bounds__(256) void kmeans_tail(double* __restrict__ out, int k, int d,
                                                   const unsigned long long* __restrict__ counts,
                                                   const double* __restrict__ cost, int64_t n) {
    const int j = threadIdx.x;
    double* tail = out + (int64_t)k * d;
    if (counts && j < k) tail[j] = (double)counts[j];
    if (j == 0) {
        tail[k] = cost[0];
        tail[k + 1] = (double)n;
    }
}

// ---- CSR ----
template <typename S, bool LDSB>
__global__ __launch_bounds__(kKmBlock) void kmeans_assign_csr(const ChainDesc* __restrict__ descs,
                                                              const KmPart* __restrict__ tab, int P, int64_t n_tiles,
                                                              KmGeom gm, const double* __restrict__ C,
                                                              const double* __restrict__ cn, int32_t* __restrict__ assign,
                                                              double* __restrict__ dist2, double* __restrict__ rec) {
    extern __shared__ double km_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = gm.d, k = gm.k, kpad = gm.kpad;
    if constexpr (LDSB) {
        const int total = d * kpad;   // C^T, its rows widened to kpad
        for (int i = (int)threadIdx.x; i < total; i += kKmBlock) {
            const int f = i / kpad, c = i - f * kpad;
            km_lds[i] = c < k ? C[(int64_t)c * d + f] : 0.0;
        }
        __syncthreads();
    }
    const int gl = gm.group, rpw = 64 / gl;
    const int g = lane / gl, j = lane & (gl - 1);
    const double inf = __builtin_inf();
    // the lane's centres; one >= k reads centre 0 and is masked at the argmin
    int comp[4];
    double cnv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        comp[c] = c * gl + j < k ? c * gl + j : 0;
        cnv[c] = cn[comp[c]];
    }
    for (int64_t tile = (int64_t)blockIdx.x * kKmWaves + wave; tile < n_tiles; tile += (int64_t)gridDim.x * kKmWaves) {
        const int p = km_partition(tab, P, tile);
        const KmPart pp = tab[p];
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - pp.tile0) * kKmCsrTile;
        const int64_t r1 = r0 + kKmCsrTile < dsc.n_rows ? r0 + kKmCsrTile : dsc.n_rows;
        if (r1 <= r0) {
            if (lane == 0) rec[tile] = 0.0;
            continue;
        }
        const S* val = reinterpret_cast<const S*>(dsc.x);
        double cost = 0.0;
        for (int64_t rb = r0; rb < r1; rb += rpw) {
            const int64_t r = rb + g;
            const bool active = r < r1;
            const int64_t rr = active ? r : r1 - 1;   // (the shuffles below take every lane)
            const int64_t b0 = dsc.row_ptr[rr], b1 = dsc.row_ptr[rr + 1];
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            double xn = 0.0;
            for (int64_t e = b0; e < b1; ++e) {
                const double v = (double)val[e];
                const int64_t col = dsc.col[e];
                xn = m_fma(v, v, xn);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c * gl >= k) break;   // (uniform)
                    double b;
                    if constexpr (LDSB)
                        b = km_lds[(int)col * kpad + comp[c]];
                    else
                        b = C[(int64_t)comp[c] * d + col];
                    acc[c] = m_fma(v, b, acc[c]);
                }
            }
            double bv = inf;
            int bi = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c * gl >= k) break;   // (uniform)
                const int idx = c * gl + j;
                const double s = idx < k ? m_fma(-2.0, acc[c], cnv[c]) : inf;
                const bool take = s < bv;
                bv = take ? s : bv;
                bi = take ? idx : bi;
            }
            for (int off = 1; off < gl; off <<= 1) {
                const double pv = __shfl_xor(bv, off);
                const int pi = __shfl_xor(bi, off);
                const bool take = pv < bv || (pv == bv && pi < bi);
                bv = take ? pv : bv;
                bi = take ? pi : bi;
            }
            if (j == 0 && active) {
                double d2 = xn + bv;
                d2 = d2 > 0.0 ? d2 : 0.0;
                assign[pp.row0 + r] = bi;
                if (dist2) dist2[pp.row0 + r] = d2;
                cost += d2;
            }
        }
        cost = wave_sum(cost);
        if (lane == 0) rec[tile] = cost;
    }
}

template <typename S, bool LDSS>
__global__ __launch_bounds__(kKmSumBlock) void kmeans_sums_csr(const ChainDesc* __restrict__ descs,
                                                               const KmPart* __restrict__ tab, int P, int64_t n_tiles,
                                                               KmGeom gm, const int32_t* __restrict__ assign,
                                                               double* sums, unsigned long long* counts) {
    extern __shared__ double km_lds[];
    __shared__ unsigned cnt_lds[kKmeansMaxK];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = gm.d, k = gm.k;
    const int kd = k * d;   // (LDSS: <= kKmLdsSums)
    if constexpr (LDSS)
        for (int i = (int)threadIdx.x; i < kd; i += kKmSumBlock) km_lds[i] = 0.0;
    for (int i = (int)threadIdx.x; i < k; i += kKmSumBlock) cnt_lds[i] = 0u;
    __syncthreads();
    const int gl = gm.sgroup, rpw = 64 / gl;
    const int g = lane / gl, j = lane & (gl - 1);
    for (int64_t tile = (int64_t)blockIdx.x * kKmSumWaves + wave; tile < n_tiles;
         tile += (int64_t)gridDim.x * kKmSumWaves) {
        const int p = km_partition(tab, P, tile);
        const KmPart pp = tab[p];
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - pp.tile0) * kKmCsrTile;
        const int64_t r1 = r0 + kKmCsrTile < dsc.n_rows ? r0 + kKmCsrTile : dsc.n_rows;
        const S* val = reinterpret_cast<const S*>(dsc.x);
        for (int64_t rb = r0; rb < r1; rb += rpw) {
            const int64_t r = rb + g;
            if (r >= r1) continue;
            const int a = assign[pp.row0 + r];
            const int64_t b0 = dsc.row_ptr[r], b1 = dsc.row_ptr[r + 1];
            for (int64_t e = b0 + j; e < b1; e += gl) {
                const double v = (double)val[e];
                const int64_t col = dsc.col[e];
                if constexpr (LDSS)
                    __hip_atomic_fetch_add(&km_lds[a * d + (int)col], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    unsafeAtomicAdd(sums + (int64_t)a * d + col, v);
            }
            if (j == 0) atomicAdd(&cnt_lds[a], 1u);
        }
    }
    __syncthreads();
    if constexpr (LDSS)
        for (int i = (int)threadIdx.x; i < kd; i += kKmSumBlock) {
            const double v = km_lds[i];
            if (v != 0.0) unsafeAtomicAdd(sums + i, v);
        }
    for (int i = (int)threadIdx.x; i < k; i += kKmSumBlock) {
        const unsigned c = cnt_lds[i];
        if (c) atomicAdd(counts + i, (unsigned long long)c);
    }
}

// Thread (j, f): the new centre's entry; an empty cluster keeps its centre.
__global__ __launch_bounds__(256) void kmeans_update(int k, int d, const double* __restrict__ C,
                                                     const double* __restrict__ step, double* __restrict__ c_new) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)k * d) return;
    const int j = (int)(i / d);
    const double cnt = step[(int64_t)k * d + j];
    c_new[i] = cnt > 0.0 ? step[i] * (1.0 / cnt) : C[i];
}

// Thread j: moved[j] = sum_f (c_new - c)^2, along the features.
__global__ __launch_bounds__(256) void kmeans_moved(int k, int d, const double* __restrict__ C,
                                                    const double* __restrict__ c_new, double* __restrict__ moved) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    double s = 0.0;
    for (int f = 0; f < d; ++f) {
        const double t = c_new[(int64_t)j * d + f] - C[(int64_t)j * d + f];
        s = m_fma(t, t, s);
    }
    moved[j] = s;
}

template <typename K, typename... A>
int km_launch(K kern, unsigned blocks, int threads, int64_t lds, hipStream_t st, A... args) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), (size_t)lds, st, args...);
    return (int)hipGetLastError();
}

template <typename S, bool LDSB, typename... A>
int assign_dense_cb(int cb, unsigned blocks, int64_t lds, hipStream_t st, A... args) {
    switch (cb) {
        case 1: return km_launch(kmeans_assign_dense<S, 1, LDSB>, blocks, kKmBlock, lds, st, args...);
        case 2: return km_launch(kmeans_assign_dense<S, 2, LDSB>, blocks, kKmBlock, lds, st, args...);
        case 4: return km_launch(kmeans_assign_dense<S, 4, LDSB>, blocks, kKmBlock, lds, st, args...);
    }
    return (int)hipErrorInvalidValue;
}

template <typename S, typename... A>
int assign_s(const KmGeom& gm, unsigned blocks, hipStream_t st, A... args) {
    if (gm.path == kKmDenseLds) return assign_dense_cb<S, true>(gm.cb, blocks, gm.lds_bytes, st, args...);
    if (gm.path == kKmDenseL2) return assign_dense_cb<S, false>(gm.cb, blocks, 0, st, args...);
    return gm.clds ? km_launch(kmeans_assign_csr<S, true>, blocks, kKmBlock, gm.lds_bytes, st, args...)
                   : km_launch(kmeans_assign_csr<S, false>, blocks, kKmBlock, 0, st, args...);
}

template <typename S, typename... A>
int sums_dense_s(const KmGeom& gm, unsigned blocks, hipStream_t st, A... args) {
    const int key = gm.gr * 16 + gm.gc;
    switch (key) {
        case 1 * 16 + 2: return km_launch(kmeans_sums_dense<S, 1, 2>, blocks, kKmSumBlock, 0, st, args...);
        case 1 * 16 + 8: return km_launch(kmeans_sums_dense<S, 1, 8>, blocks, kKmSumBlock, 0, st, args...);
        case 2 * 16 + 2: return km_launch(kmeans_sums_dense<S, 2, 2>, blocks, kKmSumBlock, 0, st, args...);
        case 2 * 16 + 8: return km_launch(kmeans_sums_dense<S, 2, 8>, blocks, kKmSumBlock, 0, st, args...);
        case 4 * 16 + 2: return km_launch(kmeans_sums_dense<S, 4, 2>, blocks, kKmSumBlock, 0, st, args...);
        case 4 * 16 + 8: return km_launch(kmeans_sums_dense<S, 4, 8>, blocks, kKmSumBlock, 0, st, args...);
    }
    return (int)hipErrorInvalidValue;
}

// The scratch of a call, in doubles: [pack | cn | tile costs | their spans | cost | records or counts].
struct KmScratch {
    int64_t cn, rec, rec2, cost, sums;
};
KmScratch km_scratch(const KmGeom& gm, int64_t n_tiles) {
    KmScratch s{};
    s.cn = gm.pack_doubles - gm.kpad;
    s.rec = gm.pack_doubles;
    const int64_t T = n_tiles > 0 ? n_tiles : 1;
    s.rec2 = s.rec + T;
    s.cost = s.rec2 + (T + grad_merge_span(T) - 1) / grad_merge_span(T);
    s.sums = s.cost + 1;
    return s;
}

unsigned zero_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024)); }

}  // namespace

KmGeom kmeans_geometry(int layout, int storage, int d, int k, int64_t n_tiles, int64_t max_nnz) {
    KmGeom gm{};
    gm.d = d;
    gm.k = k;
    gm.kpad = 16 * ((k + 15) / 16);
    gm.nb = gm.kpad / 16;
    if (layout == kCsr) {
        int gl = 1;
        while (gl < k && gl < 64) gl *= 2;
        gm.group = gl;
        gm.cb = (k + gl - 1) / gl;
        gm.sgroup = max_nnz <= 16 ? 16 : max_nnz <= 32 ? 32 : 64;
        gm.tile_rows = kKmCsrTile;
        gm.dpad = d;
        const int64_t bytes = (int64_t)d * gm.kpad * (int64_t)sizeof(double);
        gm.clds = bytes <= kKmLds;
        gm.lds_bytes = gm.clds ? bytes : 0;
        gm.path = (int64_t)k * d <= kKmLdsSums ? kKmCsrLdsSums : kKmCsrGlobalSums;
        gm.pack_doubles = gm.kpad;
        const KmScratch s = km_scratch(gm, n_tiles);
        gm.n_spans = n_tiles > 0 ? s.cost - s.rec2 : 0;
        gm.span = grad_merge_span(n_tiles > 0 ? n_tiles : 1);
        gm.assign_bytes = s.sums * (int64_t)sizeof(double);
        gm.scratch_bytes = (s.sums + k) * (int64_t)sizeof(double);   // (the counts: k 64-bit integers)
        return gm;
    }
    const int vec = storage == 1 ? 4 : 2;
    const int fchunk = 4 * vec;
    gm.dpad = (int32_t)(((int64_t)d + fchunk - 1) / fchunk * fchunk);
    gm.tile_rows = 16;
    gm.cb = gm.nb == 1 ? 1 : gm.nb == 2 ? 2 : 4;
    const int64_t bytes = (int64_t)gm.dpad * gm.kpad * (int64_t)sizeof(double);
    gm.path = bytes <= kKmLds ? kKmDenseLds : kKmDenseL2;
    gm.clds = gm.path == kKmDenseLds;
    gm.lds_bytes = gm.clds ? bytes : 0;
    gm.pack_doubles = (int64_t)gm.dpad * gm.kpad + gm.kpad;
    // the smallest built rectangle that holds the blocks, 4 x 8 (256 accumulator registers) at most
    gm.nbf = (d + 1 + 15) / 16;
    gm.gr = gm.nb == 1 ? 1 : gm.nb == 2 ? 2 : 4;
    gm.gc = gm.nbf <= 2 ? 2 : 8;
    gm.nrg = (gm.nb + gm.gr - 1) / gm.gr;
    gm.ncg = (gm.nbf + gm.gc - 1) / gm.gc;
    const int64_t n_rects = (int64_t)gm.nrg * gm.ncg;
    gm.span = 1;
    if (n_tiles > 0) {
        // about kKmItems items of 4 x 8 blocks, more of the smaller rectangles (gram_geometry's cap)
        const int64_t items = kKmItems * (gm.gr * gm.gc >= 32 ? 1 : gm.gr * gm.gc >= 8 ? 2 : 4);
        int64_t want = (items + n_rects - 1) / n_rects;
        if (want > n_tiles) want = n_tiles;
        gm.span = (n_tiles + want - 1) / want;
        gm.n_spans = (n_tiles + gm.span - 1) / gm.span;
    }
    gm.n_items = gm.n_spans * n_rects;
    const KmScratch s = km_scratch(gm, n_tiles);
    gm.assign_bytes = s.sums * (int64_t)sizeof(double);
    gm.scratch_bytes = (s.sums + gm.n_items * gm.gr * gm.gc * 256) * (int64_t)sizeof(double);
    return gm;
}

int launch_kmeans_assign(const ChainDesc* descs, const KmPart* tab, int n_parts, int64_t n_tiles, const KmGeom& gm,
                         int storage, const double* C, double* scratch, int32_t* assign, double* dist2, double* cost,
                         int num_cus, hipStream_t st) {
    const KmScratch sc = km_scratch(gm, n_tiles);
    if (n_tiles <= 0) {
        if (cost) hipLaunchKernelGGL(kmeans_zero, dim3(1), dim3(256), 0, st, cost, (int64_t)1);
        return (int)hipGetLastError();
    }
    const bool dense = gm.path == kKmDenseLds || gm.path == kKmDenseL2;
    const int64_t total = dense ? (int64_t)gm.dpad * gm.kpad : 0;
    const unsigned pb = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL(kmeans_pack_c, dim3(pb), dim3(256), 0, st, C, gm.d, gm.k, gm.nb, storage == 1 ? 4 : 2, total,
                       scratch, scratch + sc.cn);
    int e = (int)hipGetLastError();
    if (e) return e;
    // whole workgroups a CU: as many as its LDS holds, four of eight waves at most
    const int64_t per_cu = gm.lds_bytes > 0 ? std::max<int64_t>(1, std::min<int64_t>(4, kKmLds / gm.lds_bytes)) : 4;
    const unsigned blocks = (unsigned)std::min<int64_t>((n_tiles + kKmWaves - 1) / kKmWaves, per_cu * num_cus);
    const double* src = dense ? scratch : C;
    e = storage == 1 ? assign_s<float>(gm, blocks, st, descs, tab, n_parts, n_tiles, gm, src,
                                       (const double*)(scratch + sc.cn), assign, dist2, scratch + sc.rec)
                     : assign_s<double>(gm, blocks, st, descs, tab, n_parts, n_tiles, gm, src,
                                        (const double*)(scratch + sc.cn), assign, dist2, scratch + sc.rec);
    if (e || !cost) return e;
    return grad_merge_records(scratch + sc.rec, n_tiles, 1, scratch + sc.rec2, cost, st);
}

int launch_kmeans_step(const ChainDesc* descs, const KmPart* tab, int n_parts, int64_t n_tiles, int64_t n_rows,
                       const KmGeom& gm, int storage, const double* C, double* scratch, int32_t* assign, double* out,
                       int num_cus, hipStream_t st) {
    const int64_t kd = (int64_t)gm.k * gm.d;
    if (n_tiles <= 0) {
        hipLaunchKernelGGL(kmeans_zero, dim3(zero_blocks(kd + gm.k + 2)), dim3(256), 0, st, out, kd + gm.k + 2);
        return (int)hipGetLastError();
    }
    const KmScratch sc = km_scratch(gm, n_tiles);
    double* cost = scratch + sc.cost;
    int e = launch_kmeans_assign(descs, tab, n_parts, n_tiles, gm, storage, C, scratch, assign, nullptr, cost, num_cus, st);
    if (e) return e;
    double* rec = scratch + sc.sums;
    const unsigned long long* counts = nullptr;
    if (gm.path == kKmDenseLds || gm.path == kKmDenseL2) {
        const unsigned blocks = (unsigned)((gm.n_items + kKmSumWaves - 1) / kKmSumWaves);
        e = storage == 1 ? sums_dense_s<float>(gm, blocks, st, descs, tab, n_parts, n_tiles, gm, (const int32_t*)assign, rec)
                         : sums_dense_s<double>(gm, blocks, st, descs, tab, n_parts, n_tiles, gm, (const int32_t*)assign, rec);
        if (e) return e;
        hipLaunchKernelGGL(kmeans_merge, dim3((unsigned)((gm.d + 1 + kKmSumBlock - 1) / kKmSumBlock), (unsigned)gm.k),
                           dim3(kKmSumBlock), 0, st, (const double*)rec, gm, out);
    } else {
        // the accumulators start from zero: a kernel, not a memset node, so that a captured step replays
        hipLaunchKernelGGL(kmeans_zero, dim3(zero_blocks(kd)), dim3(256), 0, st, out, kd);
        hipLaunchKernelGGL(kmeans_zero, dim3(1), dim3(256), 0, st, rec, (int64_t)gm.k);
        e = (int)hipGetLastError();
        if (e) return e;
        unsigned long long* cnt = reinterpret_cast<unsigned long long*>(rec);
        counts = cnt;
        const bool lds = gm.path == kKmCsrLdsSums;
        const int64_t lds_bytes = lds ? kd * (int64_t)sizeof(double) : 0;
        const unsigned blocks = grad_balanced_blocks(n_tiles, num_cus, lds ? 2 : 8);
        if (storage == 1)
            e = lds ? km_launch(kmeans_sums_csr<float, true>, blocks, kKmSumBlock, lds_bytes, st, descs, tab, n_parts,
                                n_tiles, gm, (const int32_t*)assign, out, cnt)
                    : km_launch(kmeans_sums_csr<float, false>, blocks, kKmSumBlock, 0, st, descs, tab, n_parts, n_tiles,
                                gm, (const int32_t*)assign, out, cnt);
        else
            e = lds ? km_launch(kmeans_sums_csr<double, true>, blocks, kKmSumBlock, lds_bytes, st, descs, tab, n_parts,
                                n_tiles, gm, (const int32_t*)assign, out, cnt)
                    : km_launch(kmeans_sums_csr<double, false>, blocks, kKmSumBlock, 0, st, descs, tab, n_parts, n_tiles,
                                gm, (const int32_t*)assign, out, cnt);
    }
    if (e) return e;
    e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(kmeans_tail, dim3(1), dim3(256), 0, st, out, gm.k, gm.d, counts, (const double*)cost, n_rows);
    return (int)hipGetLastError();
}

int launch_kmeans_update(int k, int d, const double* C, const double* step, double* c_new, double* moved,
                         hipStream_t st) {
    const int64_t kd = (int64_t)k * d;
    hipLaunchKernelGGL(kmeans_update, dim3((unsigned)((kd + 255) / 256)), dim3(256), 0, st, k, d, C, step, c_new);
    int e = (int)hipGetLastError();
    if (e) return e;
    hipLaunchKernelGGL(kmeans_moved, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, k, d, C,
                       (const double*)c_new, moved);
    return (int)hipGetLastError();
}

}  // namespace psgd
