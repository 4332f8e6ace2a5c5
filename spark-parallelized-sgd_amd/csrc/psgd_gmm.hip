// psgd_gmm.hip -- one EM step of a Gaussian mixture over the registered dense partitions
// (psgd_gmm_responsibilities, psgd_gmm_moments_device, psgd_gmm_step). A model is k components; the host
// hands over A [k][d][d] (A_j[i][c] = R_j[c][i], R_j the root of the pseudo-inverse covariance), b [k][d]
// (b_j = R_j mu_j) and c [k] (c_j = ln w_j + u_j). All arithmetic is fp64 whatever the storage. For a row
// x: v_jc = -b_j[c] + sum_i x_i A_j[i][c] (one fma chain along the features that starts at -b_j[c]),
// q_j = sum_c v_jc^2, p_j = EPS + exp(c_j - q_j / 2) with EPS = 2^-52, P = sum_j p_j in ascending j,
// r_j = p_j / P; the row adds ln P to the log-likelihood. The moments are S_j = sum_rows r_j z z^T with
// z = [x, 1], (d + 1)^2 doubles a component. A step returns {S[k][d + 1][d + 1], log-likelihood, n}.
//
// Rows are cut into tiles of 16 rows numbered across the partitions in partition-index order
// (KmPart::tile0, the k-means passes' table); KmPart::row0 places a partition in the local row order of
// the responsibilities, which lie [row][k] row-major inside as outside: the E-step writes a tile's 16 k
// doubles as one contiguous run, and the moments' items of one span, which each take 8 bytes of a row's
// k, run together and meet the lines in L2.
//
// gmm_pack writes the k matrices side by side into project_pack_b's operand order: with db = ceil(d / 16)
// component j owns the column blocks [j db, (j + 1) db), nb = k db in all; index ((s nb + B) VEC + e) 64 + l
// holds A_j[(4 s + (l >> 4)) VEC + e][16 bj + (l & 15)] for B = j db + bj, zero past d either way. negb
// [16 nb] holds -b in the same column order (0.0 at a pad column), cc [k] a copy of c.
//
// E-step (gmm_estep_dense): v_mfma_f64_16x16x4_f64 with M = rows, K = features, N = the nb column blocks,
// in project_dense's geometry. An item is a 16-row tile; the wave walks chunks of CB column blocks (from
// the second chunk on its rows come from L2). Lane l = (m = l & 15, q = l >> 4) reads row m as 16-byte
// vectors at the row's own pitch; loads carry no branch, a vector past the row's last reloads the last, a
// row past the tile's end the partition's last row, a feature >= d is replaced by 0.0 by selection. The
// accumulators start at -b (the MFMA's C operand). After a chunk the lane holds D[row = q + 4 g][col = 16
// bj + m] of each block: it adds the square with fma into a running partial of q_j per row g, in ascending
// block order, a pad column left out by selection. The partial lives across chunk boundaries, so a
// component whose blocks straddle one is summed in the same order as one that does not. When block
// bj = db - 1 is done the 16 lanes of the DPP row add their partials by a butterfly (quad_perm [1,0,3,2],
// quad_perm [2,3,0,1], row_half_mirror, row_mirror: partners swap, so all 16 end with the same bits) and
// lanes m < 4 put q_j of rows q + 4 m into the wave's staging in LDS ([j][16 rows]). After the last chunk
// the 64 lanes walk the tile's 16 k pairs (row, j) in the output's order: p = EPS + exp(fma(-0.5, q, c))
// replaces q in the staging (q itself goes out when asked for); then lane (l & 15) adds its row's p_j in
// ascending j, takes ln P, and the lanes walk the pairs again for the k divisions p_j / P. exp, ln and the
// divisions therefore run once a (row, component), not once a lane of the reduction. The tile's sum of
// ln P is added in row order into one record; the records are merged in tile order
// (grad_merge_records). The packed operands lie in LDS in front of the staging while both fit a CU's
// 160 KiB, else they are read through L2. No atomics; the same bits from call to call, whatever the grid.
//
// Moments (gmm_moments_dense): gram_dense's design with M = N = the a = d + 1 columns of z and K = rows.
// For rows i0 .. i0 + 3 lane l holds z[i0 + (l >> 4)][c0 + (l & 15)]; the B operand is z as it lies, the A
// operand z * r_j of the lane's row: one rounding before the MFMA's exact products, as the weighted
// Gramian scales it. An item is (span of tiles, component, rectangle of gr x gc blocks that meets the
// upper triangle), numbered span-major, component next: the four waves of a workgroup and the
// workgroups next to it walk the same rows. An item ends in one record; gmm_merge adds the records in
// span order and writes both triangles from the upper one (inside a diagonal block too, where
// (z_a r) z_b and (z_b r) z_a differ in their last bit), so S_j == S_j^T bit for bit. A column >= d loads
// feature d - 1 by selection (a zero-copy row's pad is never read) and takes 1.0 at column d, else 0.0; a
// row past its run's end loads the run's last row and takes 0.0. No floating-point atomics; the order of
// every sum is fixed by the tiling and the plan (gmm_geometry), never by the grid.
#include <algorithm>

#include "psgd_device.h"

namespace psgd {
namespace {

constexpr int kGmBlock = 512;               // the E-step kernel, at most (gm.waves waves are launched)
constexpr int kGmU = 4;                     // steps whose vectors are loaded together (one stage)
constexpr int64_t kGmLds = 160 * 1024;      // a CU's LDS
constexpr int kGmMomBlock = 256;            // the moments kernels
constexpr int kGmMomWaves = kGmMomBlock / 64;
constexpr int kGmSub = 2;                   // 4-row steps whose fragments are loaded together (one stage)
constexpr int64_t kGmItems = 2048;          // items the moments' plan aims at
constexpr double kGmEps = 2.220446049250313e-16;   // 2^-52, MLlib's EPSILON
typedef double gm_d4 __attribute__((ext_vector_type(4)));

// The tile's partition: the last p with tab[p].tile0 <= tile. Uniform over the wave.
__device__ __forceinline__ int gm_partition(const KmPart* tab, int P, int64_t tile) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

// First kept rectangle of rectangle row R: the first whose last block column reaches the row's first block.
__host__ __device__ inline int gm_first_group(int R, int gr, int gc) { return R * gr / gc; }

__global__ __launch_bounds__(256) void gmm_zero(double* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0.0;
}

// total = dpad 16 nb operands of Ap; then negb [16 nb] and cc [k].
__global__ __launch_bounds__(256) void gmm_pack(const double* __restrict__ A, const double* __restrict__ b,
                                                const double* __restrict__ c, int d, int k, int db, int vec,
                                                int64_t total, double* __restrict__ Ap, double* __restrict__ negb,
                                                double* __restrict__ cc) {
    const int nb = k * db;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = t0; i < total; i += stride) {
        const int l = (int)(i & 63);
        int64_t t = i >> 6;
        const int e = (int)(t % vec);
        t /= vec;
        const int B = (int)(t % nb);
        const int64_t s = t / nb;
        const int64_t f = (4 * s + (l >> 4)) * vec + e;
        const int j = B / db;
        const int col = 16 * (B - j * db) + (l & 15);
        Ap[i] = f < d && col < d ? A[((int64_t)j * d + f) * d + col] : 0.0;
    }
    for (int64_t i = t0; i < 16 * (int64_t)nb; i += stride) {
        const int B = (int)(i >> 4);
        const int j = B / db;
        const int col = 16 * (B - j * db) + (int)(i & 15);
        negb[i] = col < d ? -b[(int64_t)j * d + col] : 0.0;
    }
    for (int64_t i = t0; i < k; i += stride) cc[i] = c[i];
}

template <typename S, int CB, bool LDSB>
__global__ __launch_bounds__(kGmBlock) void gmm_estep_dense(const ChainDesc* __restrict__ descs,
                                                            const KmPart* __restrict__ tab, int P, int64_t n_tiles,
                                                            GmmGeom gm, const double* __restrict__ Ap,
                                                            const double* __restrict__ negb,
                                                            const double* __restrict__ cc, double* __restrict__ resp,
                                                            double* __restrict__ qout, double* __restrict__ rec) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    extern __shared__ double gm_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int waves = (int)(blockDim.x >> 6);
    const int d = gm.d, k = gm.k, db = gm.db, nb = gm.nb;
    const int nsteps = gm.dpad / (4 * VEC);
    const int opd = LDSB ? (int)gm.op_doubles : 0;
    if constexpr (LDSB) {
        for (int i = 2 * (int)threadIdx.x; i < opd; i += 2 * (int)blockDim.x) {   // (opd is a multiple of 128)
            const f64x2 v = *reinterpret_cast<const f64x2*>(Ap + i);
            *reinterpret_cast<f64x2*>(gm_lds + i) = v;
        }
        __syncthreads();
    }
    // the wave's staging: q_j, then p_j, of the tile's rows as [j][16], and the rows' P
    double* stage = gm_lds + opd + wave * (16 * k + 16);
    double* prow = stage + 16 * k;
    const int m = lane & 15, q = lane >> 4;
    const int nvec = (d + VEC - 1) / VEC;       // the row's vectors that hold a feature (<= ld / VEC)
    const int nchunk = (nb + CB - 1) / CB;
    const int npair = 16 * k;
    for (int64_t tile = (int64_t)blockIdx.x * waves + wave; tile < n_tiles; tile += (int64_t)gridDim.x * waves) {
        const int p = gm_partition(tab, P, tile);
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
        // the running partial of q_j of rows q, q + 4, q + 8, q + 12 over this lane's columns: it lives
        // across the chunks until the component's last block
        double qp[4] = {0.0, 0.0, 0.0, 0.0};

        // A stage's loads carry no branch: a vector past the row's last loads the last (in bounds at
        // the row's own pitch), and what it holds at a feature >= d is replaced at its use.
        auto load = [&](V (&xv)[kGmU], int s0) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < kGmU; ++u) {
                const int vi = 4 * (s0 + u) + q;
                xv[u] = xr[vi < nvec ? vi : nvec - 1];
            }
        };
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            // the chunk's blocks; one past the last repeats the last and is not used
            int bi[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c) bi[c] = chunk * CB + c < nb ? chunk * CB + c : nb - 1;
            gm_d4 acc[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                const double nbv = as_global(negb)[16 * bi[c] + m];
                acc[c] = gm_d4{nbv, nbv, nbv, nbv};
            }
            auto compute = [&](const V (&xv)[kGmU], int s0) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < kGmU; ++u) {
                    const int s = s0 + u;
                    if (s >= nsteps) break;   // (uniform)
                    double a[VEC];
                    unpack<S, double>(xv[u], a);
                    const int f0 = (4 * s + q) * VEC;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) a[e] = f0 + e < d ? a[e] : 0.0;
#pragma unroll
                    for (int e = 0; e < VEC; ++e)
#pragma unroll
                        for (int c = 0; c < CB; ++c) {
                            double bv;
                            if constexpr (LDSB)
                                bv = gm_lds[((s * nb + bi[c]) * VEC + e) * 64 + lane];
                            else
                                bv = as_global(Ap)[(((int64_t)s * nb + bi[c]) * VEC + e) * 64 + lane];
                            acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], bv, acc[c], 0, 0, 0);
                        }
                }
            };
            // two sets of vectors: the next stage's loads are in flight under this stage's MFMAs
            V xa[kGmU], xb[kGmU];
            int s0 = 0;
            load(xa, 0);
            while (s0 < nsteps) {
                load(xb, s0 + kGmU);
                compute(xa, s0);
                s0 += kGmU;
                if (s0 >= nsteps) break;
                load(xa, s0 + kGmU);
                compute(xb, s0);
                s0 += kGmU;
            }
            // D[q + 4 g][16 bj + m]: the lane's column of each block against four rows, ascending blocks
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                const int blk = chunk * CB + c;
                if (blk >= nb) break;   // (uniform)
                const int j = blk / db, bj = blk - j * db;
                const bool col_on = 16 * bj + m < d;
#pragma unroll
                for (int g = 0; g < 4; ++g) qp[g] = col_on ? m_fma(acc[c][g], acc[c][g], qp[g]) : qp[g];
                if (bj == db - 1) {   // (uniform) the component is complete: over the 16 lanes of the DPP row
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        qp[g] = qp[g] + dpp_mov<0xB1>(qp[g]);    // quad_perm [1,0,3,2]
                        qp[g] = qp[g] + dpp_mov<0x4E>(qp[g]);    // quad_perm [2,3,0,1]
                        qp[g] = qp[g] + dpp_mov<0x141>(qp[g]);   // row_half_mirror
                        qp[g] = qp[g] + dpp_mov<0x140>(qp[g]);   // row_mirror
                    }
                    const double v = m == 0 ? qp[0] : m == 1 ? qp[1] : m == 2 ? qp[2] : qp[3];
                    if (m < 4) stage[j * 16 + q + 4 * m] = v;
#pragma unroll
                    for (int g = 0; g < 4; ++g) qp[g] = 0.0;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the tile's pairs (row, j) in the output's order; a row past the partition's end is computed
        // (its loads repeated the last row) and not written
        const int64_t left = dsc.n_rows - r0;
        const int nr = left < 16 ? (int)left : 16;
        const int64_t base = (pp.row0 + r0) * k;
        for (int idx = lane; idx < npair; idx += 64) {
            const int rw = idx / k, j = idx - rw * k;
            const double qv = stage[j * 16 + rw];
            if (qout && rw < nr) qout[base + idx] = qv;
            stage[j * 16 + rw] = kGmEps + exp(m_fma(-0.5, qv, as_global(cc)[j]));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // P of row l & 15 in ascending j (the four lanes of a row add the same values in the same order)
        double Pv = 0.0;
        for (int j = 0; j < k; ++j) Pv += stage[j * 16 + m];
        if (lane < 16) prow[lane] = Pv;
        double lnp = lane < nr ? log(Pv) : 0.0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int idx = lane; idx < npair; idx += 64) {
            const int rw = idx / k, j = idx - rw * k;
            const double r = stage[j * 16 + rw] / prow[rw];
            if (rw < nr) resp[base + idx] = r;
        }
        // the tile's log-likelihood in row order (rows past the end add 0.0)
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += readlane_d(lnp, r);
        if (lane == 0) rec[tile] = t;
        // (the next tile's q_j are stored after these loads: one wave's LDS accesses keep their order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

template <typename S, int GR, int GC>
__global__ __launch_bounds__(kGmMomBlock, 1) void gmm_moments_dense(const ChainDesc* __restrict__ descs,
                                                                   const KmPart* __restrict__ tab, int P,
                                                                   int64_t n_tiles, GmmGeom gm,
                                                                   const double* __restrict__ resp,
                                                                   double* __restrict__ rec) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t item = (int64_t)blockIdx.x * kGmMomWaves + wave;
    if (item >= gm.n_items) return;
    const int k = gm.k;
    const int64_t per_span = (int64_t)k * gm.n_groups;
    const int64_t span = item / per_span;
    const int rem = (int)(item - span * per_span);
    const int comp = rem / gm.n_groups;
    int left = rem - comp * gm.n_groups;
    int R = 0;
    for (;; ++R) {
        const int n = gm.ncg - gm_first_group(R, GR, GC);
        if (left < n) break;
        left -= n;
    }
    const int C = gm_first_group(R, GR, GC) + left;
    const int jb0 = R * GR, kb0 = C * GC;
    const int d = gm.d;
    // block (r, c) of the rectangle is computed when it lies in the upper triangle and inside S
    unsigned on = 0;
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c)
            if (jb0 + r <= kb0 + c && kb0 + c < gm.nbz) on |= 1u << (r * GC + c);
    on = __builtin_amdgcn_readfirstlane(on);
    const int m = lane & 15, kq = lane >> 4;
    // the lane's column of each fragment, and the feature it loads: a column >= d loads feature d - 1
    // (in bounds, never a pad column) and its value is not used
    int ca[GR], cb[GC], la[GR], lb[GC];
#pragma unroll
    for (int r = 0; r < GR; ++r) {
        ca[r] = (jb0 + r) * 16 + m;
        la[r] = ca[r] < d ? ca[r] : d - 1;
    }
#pragma unroll
    for (int c = 0; c < GC; ++c) {
        cb[c] = (kb0 + c) * 16 + m;
        lb[c] = cb[c] < d ? cb[c] : d - 1;
    }
    gm_d4 acc[GR][GC];
#pragma unroll
    for (int r = 0; r < GR; ++r)
#pragma unroll
        for (int c = 0; c < GC; ++c) acc[r][c] = gm_d4{0.0, 0.0, 0.0, 0.0};

    const int64_t t0 = span * gm.span;
    const int64_t t1 = t0 + gm.span < n_tiles ? t0 + gm.span : n_tiles;
    // the span's tiles, a partition's run of them at a time: consecutive tiles of a partition are
    // consecutive rows, walked four rows a step
    int64_t tile = t0;
    while (tile < t1) {
        const int p = gm_partition(tab, P, tile);
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
        const double* rrow = resp + pp.row0 * k + comp;
        // A stage's loads carry no branch and no conversion: a row past the run's end loads its last
        // row, and the selection at the use keeps it out of the sums.
        auto load = [&](S (&fa)[kGmSub][GR], S (&fb)[kGmSub][GC], double (&fo)[kGmSub], int64_t rb) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < kGmSub; ++s) {
                const int64_t row = rb + 4 * s + kq;
                const int64_t rr = row < r1 ? row : r1 - 1;
                const gptr<S> xr = as_global(X + rr * dsc.ld);
#pragma unroll
                for (int r = 0; r < GR; ++r) fa[s][r] = xr[la[r]];
#pragma unroll
                for (int c = 0; c < GC; ++c) fb[s][c] = xr[lb[c]];
                fo[s] = as_global(rrow)[rr * k];
            }
        };
        auto compute = [&](const S (&fa)[kGmSub][GR], const S (&fb)[kGmSub][GC], const double (&fo)[kGmSub], int64_t rb) __attribute__((always_inline)) {
            unsigned onl = __builtin_amdgcn_readfirstlane(on);
            asm volatile("" : "+s"(onl));
#pragma unroll
            for (int s = 0; s < kGmSub; ++s) {
                const bool valid = rb + 4 * s + kq < r1;
                double a[GR], b[GC];
                // (the A operand: z times the row's responsibility, then the row mask)
#pragma unroll
                for (int r = 0; r < GR; ++r) {
                    const double z = ca[r] < d ? (double)fa[s][r] : ca[r] == d ? 1.0 : 0.0;
                    const double v = z * fo[s];
                    a[r] = valid ? v : 0.0;
                }
#pragma unroll
                for (int c = 0; c < GC; ++c) {
                    const double z = cb[c] < d ? (double)fb[s][c] : cb[c] == d ? 1.0 : 0.0;
                    b[c] = valid ? z : 0.0;
                }
#pragma unroll
                for (int r = 0; r < GR; ++r)
#pragma unroll
                    for (int c = 0; c < GC; ++c)
                        if ((onl >> (r * GC + c)) & 1u)
                            acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[c], acc[r][c], 0, 0, 0);
            }
        };
        // two sets of fragments: the next stage's loads are in flight under this stage's MFMAs
        constexpr int64_t stage = 4 * kGmSub;
        S xa[kGmSub][GR], xb[kGmSub][GC], ya[kGmSub][GR], yb[kGmSub][GC];
        double xo[kGmSub], yo[kGmSub];
        int64_t rb = r0;
        load(xa, xb, xo, rb);
        while (rb < r1) {
            load(ya, yb, yo, rb + stage);
            compute(xa, xb, xo, rb);
            rb += stage;
            if (rb >= r1) break;
            load(xa, xb, xo, rb + stage);
            compute(ya, yb, yo, rb);
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

// Thread (component blockIdx.z, row ra = blockIdx.y, column cb >= ra): the spans' records of S[ra][cb] added
// in span order, written to both triangles.
__global__ __launch_bounds__(kGmMomBlock) void gmm_merge(const double* __restrict__ rec, GmmGeom gm,
                                                         double* __restrict__ out) {
    const int cb = blockIdx.x * kGmMomBlock + threadIdx.x;
    const int ra = blockIdx.y;
    const int comp = blockIdx.z;
    if (cb >= gm.a || ra > cb) return;
    const int jb = ra >> 4, kb = cb >> 4;
    const int R = jb / gm.gr, C = kb / gm.gc;
    int g = C - gm_first_group(R, gm.gr, gm.gc);
    for (int t = 0; t < R; ++t) g += gm.ncg - gm_first_group(t, gm.gr, gm.gc);
    const int64_t recsz = (int64_t)gm.gr * gm.gc * 256;
    const int64_t per_span = (int64_t)gm.k * gm.n_groups;
    const double* src = rec + ((int64_t)comp * gm.n_groups + g) * recsz +
                        (int64_t)((jb - R * gm.gr) * gm.gc + (kb - C * gm.gc)) * 256 + (ra & 15) * 16 + (cb & 15);
    double s = 0.0;
    for (int64_t sp = 0; sp < gm.n_spans; ++sp) s += src[sp * per_span * recsz];
    double* S = out + (int64_t)comp * gm.a * gm.a;
    S[(int64_t)ra * gm.a + cb] = s;
    S[(int64_t)cb * gm.a + ra] = s;
}

// A step's tail: the log-likelihood and the row count.
__global__ void gmm_tail(double* __restrict__ tail, const double* __restrict__ ll, int64_t n) {
    tail[0] = ll[0];
    tail[1] = (double)n;
}

template <typename K, typename... A>
int gm_launch(K kern, unsigned blocks, int threads, int64_t lds, hipStream_t st, A... args) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), (size_t)lds, st, args...);
    return (int)hipGetLastError();
}

template <typename S, bool LDSB, typename... A>
int estep_cb(int cb, unsigned blocks, int threads, int64_t lds, hipStream_t st, A... args) {
    switch (cb) {
        case 1: return gm_launch(gmm_estep_dense<S, 1, LDSB>, blocks, threads, lds, st, args...);
        case 2: return gm_launch(gmm_estep_dense<S, 2, LDSB>, blocks, threads, lds, st, args...);
        case 4: return gm_launch(gmm_estep_dense<S, 4, LDSB>, blocks, threads, lds, st, args...);
    }
    return (int)hipErrorInvalidValue;
}

template <typename S, typename... A>
int estep_s(const GmmGeom& gm, unsigned blocks, hipStream_t st, A... args) {
    return gm.path == kGmmDenseLds ? estep_cb<S, true>(gm.cb, blocks, 64 * gm.waves, gm.lds_bytes, st, args...)
                                   : estep_cb<S, false>(gm.cb, blocks, 64 * gm.waves, gm.lds_bytes, st, args...);
}

template <typename S, typename... A>
int moments_s(const GmmGeom& gm, unsigned blocks, hipStream_t st, A... args) {
    switch (gm.gr * 16 + gm.gc) {
        case 1 * 16 + 1: return gm_launch(gmm_moments_dense<S, 1, 1>, blocks, kGmMomBlock, 0, st, args...);
        case 1 * 16 + 2: return gm_launch(gmm_moments_dense<S, 1, 2>, blocks, kGmMomBlock, 0, st, args...);
        case 2 * 16 + 4: return gm_launch(gmm_moments_dense<S, 2, 4>, blocks, kGmMomBlock, 0, st, args...);
        case 4 * 16 + 8: return gm_launch(gmm_moments_dense<S, 4, 8>, blocks, kGmMomBlock, 0, st, args...);
    }
    return (int)hipErrorInvalidValue;
}

// The scratch of a call, in doubles: [packed A | negb | cc | tile records | their spans | log-likelihood |
// the moments' records].
struct GmScratch {
    int64_t negb, cc, rec, rec2, ll, mom;
};
GmScratch gm_scratch(const GmmGeom& gm, int64_t n_tiles) {
    GmScratch s{};
    s.negb = gm.op_doubles;
    s.cc = s.negb + 16 * (int64_t)gm.nb;
    s.rec = s.cc + 2 * (((int64_t)gm.k + 1) / 2);
    const int64_t T = n_tiles > 0 ? n_tiles : 1;
    s.rec2 = s.rec + T;
    s.ll = s.rec2 + (T + grad_merge_span(T) - 1) / grad_merge_span(T);
    s.mom = s.ll + 1;
    return s;
}

unsigned gm_zero_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024)); }

}  // namespace

GmmGeom gmm_geometry(int storage, int d, int k, int64_t n_tiles) {
    GmmGeom gm{};
    gm.d = d;
    gm.k = k;
    gm.db = (d + 15) / 16;
    gm.nb = k * gm.db;
    const int vec = storage == 1 ? 4 : 2;
    const int fchunk = 4 * vec;
    gm.dpad = (d + fchunk - 1) / fchunk * fchunk;
    gm.tile_rows = 16;
    gm.cb = gm.nb == 1 ? 1 : gm.nb == 2 ? 2 : 4;
    gm.op_doubles = (int64_t)gm.dpad * 16 * gm.nb;
    // the packed operands in front of eight waves' staging while both fit; else the staging alone, of
    // eight waves while two workgroups' fit a CU, of four beyond
    const int64_t stage8 = 8 * (16 * (int64_t)k + 16) * (int64_t)sizeof(double);
    const int64_t op_bytes = gm.op_doubles * (int64_t)sizeof(double);
    if (op_bytes + stage8 <= kGmLds) {
        gm.path = kGmmDenseLds;
        gm.waves = 8;
        gm.lds_bytes = op_bytes + stage8;
    } else {
        gm.path = kGmmDenseL2;
        gm.waves = 2 * stage8 <= kGmLds ? 8 : 4;
        gm.lds_bytes = stage8 / 8 * gm.waves;
    }
    // the moments: the smallest built rectangle that holds S's blocks, 4 x 8 (256 accumulator registers) at most
    gm.a = d + 1;
    gm.nbz = (gm.a + 15) / 16;
    if (gm.nbz == 1) { gm.gr = 1; gm.gc = 1; }
    else if (gm.nbz == 2) { gm.gr = 1; gm.gc = 2; }
    else if (gm.nbz <= 8) { gm.gr = 2; gm.gc = 4; }
    else { gm.gr = 4; gm.gc = 8; }
    gm.nrg = (gm.nbz + gm.gr - 1) / gm.gr;
    gm.ncg = (gm.nbz + gm.gc - 1) / gm.gc;
    gm.n_groups = 0;
    for (int R = 0; R < gm.nrg; ++R) gm.n_groups += gm.ncg - gm_first_group(R, gm.gr, gm.gc);
    gm.span = 1;
    if (n_tiles > 0) {
        // about kGmItems items of 4 x 8 blocks, more of the smaller rectangles (gram_geometry's cap)
        const int64_t items = kGmItems * (gm.gr * gm.gc >= 32 ? 1 : gm.gr * gm.gc >= 8 ? 2 : 4);
        const int64_t per_span = (int64_t)k * gm.n_groups;
        int64_t want = (items + per_span - 1) / per_span;
        if (want > n_tiles) want = n_tiles;
        gm.span = (n_tiles + want - 1) / want;
        gm.n_spans = (n_tiles + gm.span - 1) / gm.span;
    }
    gm.n_items = gm.n_spans * k * gm.n_groups;
    const GmScratch s = gm_scratch(gm, n_tiles);
    gm.scratch_bytes = (s.mom + gm.n_items * gm.gr * gm.gc * 256) * (int64_t)sizeof(double);
    return gm;
}

int launch_gmm_estep(const ChainDesc* descs, const KmPart* tab, int n_parts, int64_t n_tiles, const GmmGeom& gm,
                     int storage, const double* A, const double* b, const double* c, double* scratch, double* resp,
                     double* q, double* loglik, int num_cus, hipStream_t st) {
    if (n_tiles <= 0) {
        hipLaunchKernelGGL(gmm_zero, dim3(1), dim3(256), 0, st, loglik, (int64_t)1);
        return (int)hipGetLastError();
    }
    const GmScratch sc = gm_scratch(gm, n_tiles);
    const unsigned pb = (unsigned)std::max<int64_t>(1, std::min<int64_t>((gm.op_doubles + 255) / 256, 4096));
    hipLaunchKernelGGL(gmm_pack, dim3(pb), dim3(256), 0, st, A, b, c, gm.d, gm.k, gm.db, storage == 1 ? 4 : 2,
                       gm.op_doubles, scratch, scratch + sc.negb, scratch + sc.cc);
    int e = (int)hipGetLastError();
    if (e) return e;
    // whole workgroups a CU: as many as its LDS holds, four at most
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(4, kGmLds / gm.lds_bytes));
    const unsigned blocks = (unsigned)std::min<int64_t>((n_tiles + gm.waves - 1) / gm.waves, per_cu * num_cus);
    const double* Ap = scratch;
    const double* negb = scratch + sc.negb;
    const double* cc = scratch + sc.cc;
    e = storage == 1 ? estep_s<float>(gm, blocks, st, descs, tab, n_parts, n_tiles, gm, Ap, negb, cc, resp, q, scratch + sc.rec)
                     : estep_s<double>(gm, blocks, st, descs, tab, n_parts, n_tiles, gm, Ap, negb, cc, resp, q, scratch + sc.rec);
    if (e) return e;
    return grad_merge_records(scratch + sc.rec, n_tiles, 1, scratch + sc.rec2, loglik, st);
}

int launch_gmm_moments(const ChainDesc* descs, const KmPart* tab, int n_parts, int64_t n_tiles, const GmmGeom& gm,
                       int storage, const double* resp, double* scratch, double* out, hipStream_t st) {
    const int64_t len = (int64_t)gm.k * gm.a * gm.a;
    if (n_tiles <= 0) {
        hipLaunchKernelGGL(gmm_zero, dim3(gm_zero_blocks(len)), dim3(256), 0, st, out, len);
        return (int)hipGetLastError();
    }
    const GmScratch sc = gm_scratch(gm, n_tiles);
    double* rec = scratch + sc.mom;
    const unsigned blocks = (unsigned)((gm.n_items + kGmMomWaves - 1) / kGmMomWaves);
    const int e = storage == 1 ? moments_s<float>(gm, blocks, st, descs, tab, n_parts, n_tiles, gm, resp, rec)
                               : moments_s<double>(gm, blocks, st, descs, tab, n_parts, n_tiles, gm, resp, rec);
    if (e) return e;
    hipLaunchKernelGGL(gmm_merge, dim3((unsigned)((gm.a + kGmMomBlock - 1) / kGmMomBlock), (unsigned)gm.a, (unsigned)gm.k),
                       dim3(kGmMomBlock), 0, st, (const double*)rec, gm, out);
    return (int)hipGetLastError();
}

int launch_gmm_step(const ChainDesc* descs, const KmPart* tab, int n_parts, int64_t n_tiles, int64_t n_rows,
                    const GmmGeom& gm, int storage, const double* A, const double* b, const double* c, double* scratch,
                    double* resp, double* out, int num_cus, hipStream_t st) {
    const int64_t len = (int64_t)gm.k * gm.a * gm.a;
    if (n_tiles <= 0) {
        hipLaunchKernelGGL(gmm_zero, dim3(gm_zero_blocks(len + 2)), dim3(256), 0, st, out, len + 2);
        return (int)hipGetLastError();
    }
    const GmScratch sc = gm_scratch(gm, n_tiles);
    int e = launch_gmm_estep(descs, tab, n_parts, n_tiles, gm, storage, A, b, c, scratch, resp, nullptr, scratch + sc.ll,
                             num_cus, st);
    if (e) return e;
    e = launch_gmm_moments(descs, tab, n_parts, n_tiles, gm, storage, resp, scratch, out, st);
    if (e) return e;
    hipLaunchKernelGGL(gmm_tail, dim3(1), dim3(1), 0, st, out + len, (const double*)(scratch + sc.ll), n_rows);
    return (int)hipGetLastError();
}

}  // namespace psgd
