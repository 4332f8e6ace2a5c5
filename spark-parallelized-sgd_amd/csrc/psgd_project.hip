// psgd_project.hip -- the row projection over the registered partitions (psgd_project): new dense rows
// Y[r][j] = sum_i x[r][i] B[i][j], j < k, with each row's label beside them. All arithmetic is fp64
// whatever the storage; the output is f32 or f64 rows at the pitch ld_out (the fp64 result rounded
// once), columns [k, ld_out) zeros: rows psgd_register_dense_device takes as they lie.
//
// Source rows are cut into tiles of gm.tile_rows rows numbered across the partitions in
// partition-index order (ProjPart::tile0), so one launch serves every partition, as gather_dense does.
//
// Dense rows, v_mfma_f64_16x16x4_f64 with M = rows, K = features, N = components, bitwise
// reproducible. A wave owns the 16 rows of a tile and CB blocks of 16 components (an item is (tile,
// component chunk), the chunks of one tile adjacent so that the rows' second reading comes from L2) and
// walks the features once. Lane l = (m = l & 15, q = l >> 4) reads row m as 16-byte vectors at the
// row's own pitch: in step s its vector holds features (4 s + q) VEC + e, e < VEC (VEC = 4 f32, 2 f64),
// and element e is the A operand (A[m][q]) of the step's e-th MFMA. The B operand of that MFMA is then
// B[(4 s + q) VEC + e][16 b + (l & 15)]: project_pack_b writes B once into that order, widened to kpad
// = 16 ceil(k / 16) columns and dpad = 4 VEC ceil(d / 4 VEC) features with zeros, 64 consecutive
// doubles an MFMA (index ((s nb + b) VEC + e) 64 + l), so that a wave's operand is one conflict-free
// ds_read_b64 (B staged in LDS while dpad x kpad doubles fit) or one 512-byte line read through L2.
// D[row = q + 4 reg][column = l & 15] is stored by its lane. Every output is one chain along the
// features in an order fixed by (d, k, storage): the same bits from call to call. No atomics.
// Masking is gram_dense's: loads carry no lane-conditional branch; a lane whose vector lies past the
// row's last one loads the last one, a lane past the tile's last row loads the partition's last row;
// an element at a feature >= d (a zero-copy row's pad may hold NaN) is replaced by 0.0 by selection,
// never multiplied away; rows past the end are dropped at the store.
//
// CSR rows: a row goes to a group of gl lanes (the power of two >= k, at most 64), lane j of the
// group keeps components j, j + gl, .. (four at most: k <= 256) and adds x B[col][component] with
// fma in entry order, B's rows read from LDS while d x kpad doubles fit, else through L2 from the
// caller's matrix. Absent entries are zeros; no atomics; the same bits from call to call.
#include <algorithm>

#include "psgd_device.h"

namespace psgd {
namespace {

constexpr int kProjBlock = 512;
constexpr int kProjWaves = kProjBlock / 64;
constexpr int kProjU = 4;                    // steps whose vectors are loaded together (one stage)
constexpr int64_t kProjLds = 160 * 1024;     // a CU's LDS
constexpr int kProjCsrTile = 256;            // CSR rows a tile
typedef double proj_d4 __attribute__((ext_vector_type(4)));

// The tile's partition: the last p with tab[p].tile0 <= tile (empty partitions share their first tile
// with the next one). Uniform over the wave.
__device__ __forceinline__ int proj_partition(const ProjPart* tab, int P, int64_t tile) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].tile0 <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

// Bp[((s nb + b) VEC + e) 64 + l] = B[(4 s + (l >> 4)) VEC + e][16 b + (l & 15)], zero past d or k.
__global__ __launch_bounds__(256) void project_pack_b(const double* __restrict__ B, int d, int k, int nb, int vec,
                                                      int64_t total, double* __restrict__ Bp) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int l = (int)(i & 63);
        int64_t t = i >> 6;
        const int e = (int)(t % vec);
        t /= vec;
        const int b = (int)(t % nb);
        const int64_t s = t / nb;
        const int64_t f = (4 * s + (l >> 4)) * vec + e;
        const int c = 16 * b + (l & 15);
        Bp[i] = f < d && c < k ? B[f * k + c] : 0.0;
    }
}

template <typename S, typename O, int CB, bool LDSB>
__global__ __launch_bounds__(kProjBlock) void project_dense(const ChainDesc* __restrict__ descs,
                                                            const ProjPart* __restrict__ tab, int P,
                                                            int64_t n_tiles, ProjGeom gm,
                                                            const double* __restrict__ Bp, int64_t ld_out) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    extern __shared__ double proj_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = gm.d, k = gm.k, nb = gm.nb;
    const int nsteps = gm.dpad / (4 * VEC);
    if constexpr (LDSB) {
        const int total = gm.dpad * gm.kpad;   // a multiple of 128
        for (int i = 2 * (int)threadIdx.x; i < total; i += 2 * kProjBlock) {
            const f64x2 v = *reinterpret_cast<const f64x2*>(Bp + i);
            *reinterpret_cast<f64x2*>(proj_lds + i) = v;
        }
        __syncthreads();
    }
    const int m = lane & 15, q = lane >> 4;
    const int nvec = (d + VEC - 1) / VEC;       // the row's vectors that hold a feature (<= ld / VEC)
    const int nchunk = (nb + CB - 1) / CB;
    const int64_t n_items = n_tiles * nchunk;
    for (int64_t item = (int64_t)blockIdx.x * kProjWaves + wave; item < n_items;
         item += (int64_t)gridDim.x * kProjWaves) {
        const int64_t tile = item / nchunk;
        const int chunk = (int)(item - tile * nchunk);
        const int p = proj_partition(tab, P, tile);
        const ProjPart pp = tab[p];
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - pp.tile0) * 16;
        if (r0 >= dsc.n_rows) continue;
        const int64_t row = r0 + m;
        const int64_t rr = row < dsc.n_rows ? row : dsc.n_rows - 1;
        const gptr<V> xr = as_global(reinterpret_cast<const V*>(reinterpret_cast<const S*>(dsc.x) + rr * dsc.ld));
        // the chunk's blocks; one past B's last repeats the last and is not stored
        int bi[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) bi[c] = chunk * CB + c < nb ? chunk * CB + c : nb - 1;
        proj_d4 acc[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[c] = proj_d4{0.0, 0.0, 0.0, 0.0};

        // A stage's loads carry no branch: a vector past the row's last loads the last (in bounds at
        // the row's own pitch), and what it holds at a feature >= d is replaced at its use.
        auto load = [&](V (&xv)[kProjU], int s0) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < kProjU; ++u) {
                const int vi = 4 * (s0 + u) + q;
                xv[u] = xr[vi < nvec ? vi : nvec - 1];
            }
        };
        auto compute = [&](const V (&xv)[kProjU], int s0) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < kProjU; ++u) {
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
                        double b;
                        if constexpr (LDSB)
                            b = proj_lds[((s * nb + bi[c]) * VEC + e) * 64 + lane];
                        else
                            b = as_global(Bp)[(((int64_t)s * nb + bi[c]) * VEC + e) * 64 + lane];
                        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], b, acc[c], 0, 0, 0);
                    }
            }
        };
        // two sets of vectors: the next stage's loads are in flight under this stage's MFMAs
        V xa[kProjU], xb[kProjU];
        int s0 = 0;
        load(xa, 0);
        while (s0 < nsteps) {
            load(xb, s0 + kProjU);
            compute(xa, s0);
            s0 += kProjU;
            if (s0 >= nsteps) break;
            load(xa, s0 + kProjU);
            compute(xb, s0);
            s0 += kProjU;
        }

        // D[q + 4 reg][m]: the lane's column of each block, four rows
        O* out = reinterpret_cast<O*>(pp.x);
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            const int blk = chunk * CB + c;
            const int col = blk * 16 + m;
            if (blk < nb && col < ld_out) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int64_t r = r0 + q + 4 * g;
                    if (r < dsc.n_rows) out[r * ld_out + col] = col < k ? (O)acc[c][g] : O(0);
                }
            }
        }
        if (chunk == 0 && pp.y != nullptr && lane < 16 && row < dsc.n_rows) pp.y[row] = dsc.y[row];
        // the pad past B's last block, by the wave of the last chunk
        if (chunk == nchunk - 1) {
            for (int64_t col = (int64_t)nb * 16 + m; col < ld_out; col += 16) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int64_t r = r0 + q + 4 * g;
                    if (r < dsc.n_rows) out[r * ld_out + col] = O(0);
                }
            }
        }
    }
}

template <typename S, typename O, bool LDSB>
__global__ __launch_bounds__(kProjBlock) void project_csr(const ChainDesc* __restrict__ descs,
                                                          const ProjPart* __restrict__ tab, int P, int64_t n_tiles,
                                                          ProjGeom gm, const double* __restrict__ B, int64_t ld_out) {
    extern __shared__ double proj_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = gm.d, k = gm.k, kpad = gm.kpad;
    if constexpr (LDSB) {
        const int total = d * kpad;
        for (int i = (int)threadIdx.x; i < total; i += kProjBlock) {
            const int f = i / kpad, c = i - f * kpad;
            proj_lds[i] = c < k ? B[(int64_t)f * k + c] : 0.0;
        }
        __syncthreads();
    }
    const int gl = gm.group, rpw = 64 / gl;
    const int g = lane / gl, j = lane & (gl - 1);
    // the lane's components; one >= k reads column 0 and is not stored
    int comp[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) comp[c] = c * gl + j < k ? c * gl + j : 0;
    for (int64_t tile = (int64_t)blockIdx.x * kProjWaves + wave; tile < n_tiles;
         tile += (int64_t)gridDim.x * kProjWaves) {
        const int p = proj_partition(tab, P, tile);
        const ProjPart pp = tab[p];
        const ChainDesc dsc = descs[p];
        const int64_t r0 = (tile - pp.tile0) * kProjCsrTile;
        const int64_t r1 = r0 + kProjCsrTile < dsc.n_rows ? r0 + kProjCsrTile : dsc.n_rows;
        const S* val = reinterpret_cast<const S*>(dsc.x);
        O* out = reinterpret_cast<O*>(pp.x);
        for (int64_t rb = r0; rb < r1; rb += rpw) {
            const int64_t r = rb + g;
            if (r >= r1) continue;
            const int64_t b0 = dsc.row_ptr[r], b1 = dsc.row_ptr[r + 1];
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int64_t e = b0; e < b1; ++e) {
                const double v = (double)val[e];
                const int64_t col = dsc.col[e];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c * gl >= k) break;   // (uniform)
                    double b;
                    if constexpr (LDSB)
                        b = proj_lds[(int)col * kpad + comp[c]];
                    else
                        b = B[col * k + comp[c]];
                    acc[c] = m_fma(v, b, acc[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t oc = c * gl + j;
                if (oc < ld_out) out[r * ld_out + oc] = oc < k ? (O)acc[c] : O(0);
            }
            for (int64_t oc = 4 * gl + j; oc < ld_out; oc += gl) out[r * ld_out + oc] = O(0);
            if (j == 0 && pp.y != nullptr) pp.y[r] = dsc.y[r];
        }
    }
}

template <typename K>
int proj_launch(K kern, unsigned blocks, int64_t lds, hipStream_t st, const ChainDesc* descs, const ProjPart* tab,
                int P, int64_t n_tiles, const ProjGeom& gm, const double* B, int64_t ld_out) {
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kProjBlock), (size_t)lds, st, descs, tab, P, n_tiles, gm, B, ld_out);
    return (int)hipGetLastError();
}

template <typename S, typename O, bool LDSB>
int launch_dense_so(unsigned blocks, hipStream_t st, const ChainDesc* descs, const ProjPart* tab, int P,
                    int64_t n_tiles, const ProjGeom& gm, const double* Bp, int64_t ld_out) {
    switch (gm.cb) {
        case 1: return proj_launch(project_dense<S, O, 1, LDSB>, blocks, gm.lds_bytes, st, descs, tab, P, n_tiles, gm, Bp, ld_out);
        case 2: return proj_launch(project_dense<S, O, 2, LDSB>, blocks, gm.lds_bytes, st, descs, tab, P, n_tiles, gm, Bp, ld_out);
        case 4: return proj_launch(project_dense<S, O, 4, LDSB>, blocks, gm.lds_bytes, st, descs, tab, P, n_tiles, gm, Bp, ld_out);
    }
    return (int)hipErrorInvalidValue;
}

template <typename S, typename O>
int launch_so(unsigned blocks, hipStream_t st, const ChainDesc* descs, const ProjPart* tab, int P, int64_t n_tiles,
              const ProjGeom& gm, const double* B, int64_t ld_out) {
    switch (gm.path) {
        case kProjDenseLds: return launch_dense_so<S, O, true>(blocks, st, descs, tab, P, n_tiles, gm, B, ld_out);
        case kProjDenseL2: return launch_dense_so<S, O, false>(blocks, st, descs, tab, P, n_tiles, gm, B, ld_out);
        case kProjCsrLds: return proj_launch(project_csr<S, O, true>, blocks, gm.lds_bytes, st, descs, tab, P, n_tiles, gm, B, ld_out);
        case kProjCsrL2: return proj_launch(project_csr<S, O, false>, blocks, gm.lds_bytes, st, descs, tab, P, n_tiles, gm, B, ld_out);
    }
    return (int)hipErrorInvalidValue;
}

}  // namespace

ProjGeom project_geometry(int layout, int storage, int d, int k, int64_t max_nnz) {
    (void)max_nnz;   // (the CSR rows' lengths change no decision: a lane group walks any row)
    ProjGeom gm{};
    gm.d = d;
    gm.k = k;
    gm.kpad = 16 * ((k + 15) / 16);
    gm.nb = gm.kpad / 16;
    if (layout == kCsr) {
        int gl = 1;
        while (gl < k && gl < 64) gl *= 2;
        gm.group = gl;
        gm.rows_wave = 64 / gl;
        gm.cb = (k + gl - 1) / gl;
        gm.tile_rows = kProjCsrTile;
        gm.dpad = d;
        const int64_t bytes = (int64_t)d * gm.kpad * (int64_t)sizeof(double);
        gm.path = bytes <= kProjLds ? kProjCsrLds : kProjCsrL2;
        gm.lds_bytes = gm.path == kProjCsrLds ? bytes : 0;
        return gm;
    }
    const int vec = storage == 1 ? 4 : 2;
    gm.fchunk = 4 * vec;
    gm.dpad = (int32_t)(((int64_t)d + gm.fchunk - 1) / gm.fchunk * gm.fchunk);
    gm.rows_wave = 16;
    gm.tile_rows = 16;
    gm.cb = gm.nb == 1 ? 1 : gm.nb == 2 ? 2 : 4;
    const int64_t bytes = (int64_t)gm.dpad * gm.kpad * (int64_t)sizeof(double);
    gm.path = bytes <= kProjLds ? kProjDenseLds : kProjDenseL2;
    gm.lds_bytes = gm.path == kProjDenseLds ? bytes : 0;
    gm.scratch_bytes = bytes;
    return gm;
}

int launch_project(const ChainDesc* descs, const ProjPart* tab, int n_parts, int64_t n_tiles, const ProjGeom& gm,
                   int storage, int out_storage, const double* B, double* Bp, int64_t ld_out, int num_cus,
                   hipStream_t st) {
    if (n_tiles <= 0) return 0;
    const bool dense = gm.path == kProjDenseLds || gm.path == kProjDenseL2;
    const double* src = B;
    if (dense) {
        const int64_t total = (int64_t)gm.dpad * gm.kpad;
        const unsigned pb = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
        hipLaunchKernelGGL(project_pack_b, dim3(pb), dim3(256), 0, st, B, gm.d, gm.k, gm.nb, storage == 1 ? 4 : 2, total, Bp);
        const int e = (int)hipGetLastError();
        if (e) return e;
        src = Bp;
    }
    // whole workgroups a CU: as many as its LDS holds, four of eight waves at most
    const int64_t per_cu = gm.lds_bytes > 0 ? std::max<int64_t>(1, std::min<int64_t>(4, kProjLds / gm.lds_bytes)) : 4;
    const int64_t n_items = dense ? n_tiles * ((gm.nb + gm.cb - 1) / gm.cb) : n_tiles;
    const unsigned blocks = (unsigned)std::min<int64_t>((n_items + kProjWaves - 1) / kProjWaves, per_cu * num_cus);
    if (storage == 1)
        return out_storage == 1 ? launch_so<float, float>(blocks, st, descs, tab, n_parts, n_tiles, gm, src, ld_out)
                                : launch_so<float, double>(blocks, st, descs, tab, n_parts, n_tiles, gm, src, ld_out);
    return out_storage == 1 ? launch_so<double, float>(blocks, st, descs, tab, n_parts, n_tiles, gm, src, ld_out)
                            : launch_so<double, double>(blocks, st, descs, tab, n_parts, n_tiles, gm, src, ld_out);
}

}  // namespace psgd
