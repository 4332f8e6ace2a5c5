// psgd_eval_mn.hip -- scoring a multinomial logistic model (LogisticGradient, numClasses = K > 2) at
// fixed weights over the registered partitions (psgd_evaluate_multinomial, psgd_predict_multinomial,
// psgd_confusion*): every row's K - 1 margins in fp64, MLlib 1.6.1's predictPoint class, and the
// loss the head of psgd_multinomial.hip defines (oracle/psgd_ref.py::multinomial), summed per
// partition by psgd_eval.hip's eval_reduce over the same tiles (EvalPart).
//
// No chain: a wave takes (partition, tile) items in turn, as score_dense does. A row is read from
// HBM once, with non-temporal loads, into registers -- `gl` lanes across a row, each holding up to
// kMnHold of its elements as doubles, kMnRows rows a group -- and the class loop runs over the held
// elements: class c's dot is the same fma sequence over the lane's elements and the same group_sum
// whatever c is, so bit-identical weight blocks give bit-identical margins. Rows longer than one
// hold (gl = 64 lanes x kMnHold elements) are taken in column chunks; the margins accumulate in the
// wave's own LDS buffer, chunk by chunk, in chunk order.
//
// LDS of a workgroup: [the class blocks as f64 at a pitch dp of whole 16-byte row vectors (zeros past
// d), when (K - 1) dp <= kMnWLds | one
// margin buffer per wave]. The budget is 48 KiB of weights beside 8 waves x 3 KiB of margins =
// 72 KiB: two workgroups of 8 waves a CU (144 of its 160 KiB), 4 waves a SIMD, which the kernels'
// registers (<= 128) allow. Past kMnWLds the weights are read from L2 / HBM.
//
// The softmax bookkeeping (K - 1 exp and one log1p a row) runs when the wave's margin buffer is
// full: with K - 1 <= kMnLaneClasses the buffer holds up to 64 rows at an odd pitch and lane i
// takes row i, classes in order (the reference's order); with more classes the buffer holds the
// kMnRows rows of one pass, K - 1 doubles each, and the wave takes a row at a time, lanes across
// the classes (maximum, first index on ties, and the sum of exponentials by wave reductions).
//
// Determinism as in psgd_eval.hip: a tile's sums are fixed by the partition's own shape and K; no
// floating-point atomics. confusion_count uses integer atomics only: exact in any order.
#include "psgd_device.h"
#include "psgd_eval.h"

namespace psgd {
namespace {

constexpr int kMnWaves = 8;            // waves of a workgroup (the wide softmax launches fewer)
constexpr int kConfBlock = 256;

// What a wave needs to score the rows its margin buffer holds.
struct MnOut {
    const double* y;        // the partition's labels
    double* classes;        // nullable: [n_rows]
    double* margins;        // nullable: [n_rows * C1]
    int C1;                 // K - 1
};

// Row-per-lane: rows buf_row .. buf_row + n (n <= 64) at marg[i * pitch + c]; lane i scores row i.
__device__ __forceinline__ void mn_flush_rows(const double* marg, int n, int pitch, const MnOut& o, int64_t buf_row,
                                              int lane, double& loss_acc, double& ok_acc) {
    wave_lds_sync();
    const int C1 = o.C1;
    if (lane < n) {
        const double* m = marg + lane * pitch;
        const double y = o.y[buf_row + lane];
        const int ly = mn_d2i(y) - 1;
        double marginY = 0.0, M = -__builtin_inf(), pmax = 0.0;
        int maxIdx = 0, best = 0;
        for (int c = 0; c < C1; ++c) {
            const double v = m[c];
            if (c == ly) marginY = v;
            if (v > M) {
                M = v;
                maxIdx = c;
            }
            if (v > pmax) {   // predictPoint: the pivot wins unless a margin is positive
                pmax = v;
                best = c + 1;
            }
        }
        const bool shift = M > 0.0;
        double sum = 0.0;
        for (int c = 0; c < C1; ++c) {
            if (shift) sum = sum + (c == maxIdx ? exp(-M) : exp(m[c] - M));
            else sum = sum + exp(m[c]);
        }
        loss_acc += mn_loss(sum, marginY, M, y);
        const double pred = (double)best;
        ok_acc += pred == y ? 1.0 : 0.0;
        if (o.classes) o.classes[buf_row + lane] = pred;
    }
    if (o.margins) {
        double* out = o.margins + buf_row * C1;
        for (int q = lane; q < n * C1; q += 64) out[q] = marg[(q / C1) * pitch + q % C1];
    }
    wave_lds_sync();
}

// Lanes across the classes: rows buf_row .. buf_row + n at marg[i * C1 + c], a row at a time.
__device__ __forceinline__ void mn_flush_wide(const double* marg, int n, const MnOut& o, int64_t buf_row, int lane,
                                              double& loss_acc, double& ok_acc) {
    wave_lds_sync();
    const int C1 = o.C1;
    for (int i = 0; i < n; ++i) {
        const double* m = marg + (int64_t)i * C1;
        const double y = o.y[buf_row + i];
        const int ly = mn_d2i(y) - 1;
        double M = -__builtin_inf();
        int maxIdx = 0x7fffffff;
        for (int c = lane; c < C1; c += 64) {
            const double v = m[c];
            if (v > M) {
                M = v;
                maxIdx = c;
            }
        }
        // the maximum, the lowest class among equals
        for (int s = 1; s < 64; s <<= 1) {
            const double vo = __shfl_xor(M, s, 64);
            const int io = __shfl_xor(maxIdx, s, 64);
            if (vo > M || (vo == M && io < maxIdx)) {
                M = vo;
                maxIdx = io;
            }
        }
        if (maxIdx == 0x7fffffff) maxIdx = 0;   // (no margin compares: NaNs)
        const bool shift = M > 0.0;
        double part = 0.0;
        for (int c = lane; c < C1; c += 64) {
            if (shift) part = part + (c == maxIdx ? exp(-M) : exp(m[c] - M));
            else part = part + exp(m[c]);
        }
        const double sum = wave_sum(part);
        const double marginY = (ly >= 0 && ly < C1) ? m[ly] : 0.0;
        const double pred = shift ? (double)(maxIdx + 1) : 0.0;
        if (lane == 0) {
            loss_acc += mn_loss(sum, marginY, M, y);
            ok_acc += pred == y ? 1.0 : 0.0;
            if (o.classes) o.classes[buf_row + i] = pred;
        }
    }
    if (o.margins) {
        double* out = o.margins + buf_row * C1;
        for (int q = lane; q < n * C1; q += 64) out[q] = marg[q];
    }
    wave_lds_sync();
}

// Dense rows. d features, C1 = K - 1 class blocks; mb = doubles of a wave's margin buffer; wpad =
// doubles the weights take in LDS (WLDS).
template <typename S, bool WLDS, bool ROWLANE>
__global__ __launch_bounds__(kMnWaves * 64) void score_dense_mn(const ChainDesc* __restrict__ descs,
                                                                const EvalPart* __restrict__ ep, int P,
                                                                int64_t n_items, const double* __restrict__ w,
                                                                int d, int C1, int mb, int wpad,
                                                                double* __restrict__ tile_loss,
                                                                double* __restrict__ tile_ok,
                                                                double* __restrict__ classes,
                                                                double* __restrict__ margins) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int XH = kMnHold / VEC;   // vectors of a row a lane holds
    constexpr int R = kMnRows;
    extern __shared__ __attribute__((aligned(16))) double mn_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_waves = (int)(blockDim.x >> 6);
    const int nvec = (d + VEC - 1) / VEC;   // vectors that hold a row's d features
    const int dp = nvec * VEC;              // a class block's pitch in LDS: whole vectors, zeros past d
    if constexpr (WLDS) {
        for (int i = threadIdx.x; i < C1 * dp; i += blockDim.x) {
            const int c = i / dp, f = i - c * dp;
            mn_lds[i] = f < d ? w[(int64_t)c * d + f] : 0.0;
        }
        __syncthreads();
    }
    double* marg = mn_lds + (WLDS ? wpad : 0) + (int64_t)wave * mb;
    const int64_t base = ep[0].tile0;
    for (int64_t item = (int64_t)blockIdx.x * n_waves + wave; item < n_items;
         item += (int64_t)gridDim.x * n_waves) {
        const int p = item_partition(ep, P, item);
        const ChainDesc dsc = descs[p];
        // lanes across a row: the power of two whose hold covers the row's pitch, 64 at most
        int gl = 1;
        while (gl < 64 && (int64_t)gl * XH * 16 < dsc.ld * (int64_t)sizeof(S)) gl *= 2;
        int pitch, rp, nb;
        mn_buffer_shape<ROWLANE>(C1, 64 / gl, R, pitch, rp, nb);
        const int g = lane / gl, j = lane & (gl - 1);
        const int n_chunks = (nvec + gl * XH - 1) / (gl * XH);
        const int64_t r0 = (item - (ep[p].tile0 - base)) * ep[p].tile_rows;
        const int64_t r1 = r0 + ep[p].tile_rows < dsc.n_rows ? r0 + ep[p].tile_rows : dsc.n_rows;
        const S* X = reinterpret_cast<const S*>(dsc.x);
        const MnOut out{dsc.y, classes, margins, C1};
        int64_t buf_row = r0;   // the partition row of the buffer's first row
        double loss_acc = 0.0, ok_acc = 0.0;
        for (int64_t rb = r0; rb < r1; rb += (int64_t)rp * R) {
            bool valid[R];
            const V* row[R];
            int slot[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int64_t r = rb + (int64_t)u * rp + g;
                valid[u] = g < rp && r < r1;
                const int64_t rr = valid[u] ? r : r0;   // (a group past the tile's end re-reads its first row)
                row[u] = reinterpret_cast<const V*>(X + rr * dsc.ld);
                slot[u] = (int)(rr - buf_row) * pitch;
            }
            for (int ch = 0; ch < n_chunks; ++ch) {
                // the lane's vectors of this chunk: ch * gl * XH + t * gl + j, a wave instruction
                // reading gl * 16 contiguous bytes of each row
                V xv[R][XH];
                int eo[kMnHold];   // the held elements' features (0 for an element outside the row: its x is 0.0)
                bool in[kMnHold];
#pragma unroll
                for (int t = 0; t < XH; ++t) {
                    const int v = (ch * XH + t) * gl + j;
                    const int vv = v < nvec ? v : 0;
#pragma unroll
                    for (int u = 0; u < R; ++u) xv[u][t] = __builtin_nontemporal_load(as_global(row[u] + vv));
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const int f = v * VEC + e;
                        in[t * VEC + e] = v < nvec && f < d;   // (the last vector's tail lies in the row's pad)
                        eo[t * VEC + e] = in[t * VEC + e] ? f : 0;
                    }
                }
                double x[R][kMnHold];
#pragma unroll
                for (int u = 0; u < R; ++u)
#pragma unroll
                    for (int t = 0; t < XH; ++t) {
                        double xe[VEC];
                        unpack<S, double>(xv[u][t], xe);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) x[u][t * VEC + e] = in[t * VEC + e] ? xe[e] : 0.0;
                    }
#pragma unroll 1
                for (int c = 0; c < C1; ++c) {
                    double acc[R];
#pragma unroll
                    for (int u = 0; u < R; ++u) acc[u] = 0.0;
#pragma unroll
                    for (int t = 0; t < XH; ++t) {
                        double wk[VEC];
                        if constexpr (WLDS) {
                            // 16-byte reads: dp and the vector's first feature are even
                            const f64x2* wp = reinterpret_cast<const f64x2*>(mn_lds + c * dp + eo[t * VEC]);
#pragma unroll
                            for (int h = 0; h < VEC / 2; ++h) {
                                const f64x2 w2 = wp[h];
                                wk[2 * h] = w2[0];
                                wk[2 * h + 1] = w2[1];
                            }
                        } else {
#pragma unroll
                            for (int e = 0; e < VEC; ++e) wk[e] = w[(int64_t)c * d + eo[t * VEC + e]];
                        }
#pragma unroll
                        for (int e = 0; e < VEC; ++e)
#pragma unroll
                            for (int u = 0; u < R; ++u) acc[u] = __builtin_fma(x[u][t * VEC + e], wk[e], acc[u]);
                    }
                    static_assert(R == 2, "group_sum2 reduces the two rows of a group together");
                    group_sum2(acc[0], acc[1], gl);
#pragma unroll
                    for (int u = 0; u < R; ++u) {
                        const double dot = acc[u];
                        if (valid[u] && j == 0) {
                            double* mp = marg + slot[u] + c;
                            *mp = ch == 0 ? dot : *mp + dot;   // (the lane's own earlier store)
                        }
                    }
                }
            }
            const int64_t next = rb + (int64_t)rp * R;
            if (next - buf_row >= nb || next >= r1) {
                const int64_t end = next < r1 ? next : r1;
                if constexpr (ROWLANE) mn_flush_rows(marg, (int)(end - buf_row), pitch, out, buf_row, lane, loss_acc, ok_acc);
                else mn_flush_wide(marg, (int)(end - buf_row), out, buf_row, lane, loss_acc, ok_acc);
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

// CSR rows: one row per group of gl lanes (the partition's EvalPart::group), a lane holding up to
// kMnCsrHold of its entries (col, val as f64); rows longer than gl * kMnCsrHold entries in chunks.
// The weights are gathered from L2 / HBM: W[c * d + col]. A row without non-zeros has every margin 0.
template <typename S, bool ROWLANE>
__global__ __launch_bounds__(kMnWaves * 64) void score_csr_mn(const ChainDesc* __restrict__ descs,
                                                              const EvalPart* __restrict__ ep, int P,
                                                              int64_t n_items, const double* __restrict__ w, int d,
                                                              int C1, int mb, double* __restrict__ tile_loss,
                                                              double* __restrict__ tile_ok,
                                                              double* __restrict__ classes,
                                                              double* __restrict__ margins) {
    constexpr int H = kMnCsrHold;
    extern __shared__ __attribute__((aligned(16))) double mn_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_waves = (int)(blockDim.x >> 6);
    double* marg = mn_lds + (int64_t)wave * mb;
    const int64_t base = ep[0].tile0;
    for (int64_t item = (int64_t)blockIdx.x * n_waves + wave; item < n_items;
         item += (int64_t)gridDim.x * n_waves) {
        const int p = item_partition(ep, P, item);
        const ChainDesc dsc = descs[p];
        const int gl = ep[p].group;
        int pitch, rp, nb;
        mn_buffer_shape<ROWLANE>(C1, 64 / gl, 1, pitch, rp, nb);
        const int g = lane / gl, j = lane & (gl - 1);
        const int64_t r0 = (item - (ep[p].tile0 - base)) * ep[p].tile_rows;
        const int64_t r1 = r0 + ep[p].tile_rows < dsc.n_rows ? r0 + ep[p].tile_rows : dsc.n_rows;
        const S* val = reinterpret_cast<const S*>(dsc.x);
        const MnOut out{dsc.y, classes, margins, C1};
        int64_t buf_row = r0;
        double loss_acc = 0.0, ok_acc = 0.0;
        for (int64_t rb = r0; rb < r1; rb += rp) {
            const int64_t r = rb + g;
            const bool valid = g < rp && r < r1;
            const int64_t rr = valid ? r : r0;
            const int64_t s = dsc.row_ptr[rr];
            const int64_t e = valid ? dsc.row_ptr[rr + 1] : s;
            const int slot = (int)(rr - buf_row) * pitch;
            // every group of the wave loops over the chunks of the wave's longest row
            int64_t len = e - s;
            for (int m = 32; m >= 1; m >>= 1) {
                const int64_t o = __shfl_xor(len, m, 64);
                len = o > len ? o : len;
            }
            const int n_chunks = len > 0 ? (int)((len + (int64_t)gl * H - 1) / ((int64_t)gl * H)) : 1;
            for (int ch = 0; ch < n_chunks; ++ch) {
                double x[H];
                int col[H];
#pragma unroll
                for (int t = 0; t < H; ++t) {
                    const int64_t k = s + ((int64_t)ch * H + t) * gl + j;
                    const bool in = k < e;
                    x[t] = in ? (double)__builtin_nontemporal_load(as_global(val + k)) : 0.0;
                    col[t] = in ? __builtin_nontemporal_load(as_global(dsc.col + k)) : 0;
                }
                for (int c = 0; c < C1; ++c) {
                    const double* wc = w + (int64_t)c * d;
                    double acc = 0.0;
#pragma unroll
                    for (int t = 0; t < H; ++t) acc = __builtin_fma(x[t], wc[col[t]], acc);
                    const double dot = group_sum(acc, gl);
                    if (valid && j == 0) {
                        double* mp = marg + slot + c;
                        *mp = ch == 0 ? dot : *mp + dot;   // (the lane's own earlier store)
                    }
                }
            }
            const int64_t next = rb + rp;
            if (next - buf_row >= nb || next >= r1) {
                const int64_t end = next < r1 ? next : r1;
                if constexpr (ROWLANE) mn_flush_rows(marg, (int)(end - buf_row), pitch, out, buf_row, lane, loss_acc, ok_acc);
                else mn_flush_wide(marg, (int)(end - buf_row), out, buf_row, lane, loss_acc, ok_acc);
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

// (label, prediction) pairs into counts[label * K + prediction]; a pair with a value that is not a
// whole number in [0, K) goes to *n_bad instead. LDS: a table of the workgroup's own (K * K <=
// kConfLdsCells), flushed with 64-bit integer atomics; else the atomics go to `counts` directly.
template <bool LDS>
__global__ __launch_bounds__(kConfBlock) void confusion_count(const double* __restrict__ pred,
                                                              const double* __restrict__ lab, int64_t n, int K,
                                                              unsigned long long* __restrict__ counts,
                                                              unsigned long long* __restrict__ n_bad) {
    __shared__ unsigned long long table[LDS ? kConfLdsCells : 1];
    __shared__ unsigned long long bad_sh;
    const int cells = K * K;
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < cells; i += kConfBlock) table[i] = 0;
    }
    if (threadIdx.x == 0) bad_sh = 0;
    __syncthreads();
    const double Kd = (double)K;
    unsigned long long bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kConfBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kConfBlock) {
        const double a = lab[i], b = pred[i];
        const bool ok = a >= 0.0 && a < Kd && a == __builtin_floor(a) && b >= 0.0 && b < Kd && b == __builtin_floor(b);
        if (!ok) {
            ++bad;
            continue;
        }
        const int cell = (int)a * K + (int)b;
        if constexpr (LDS) atomicAdd(&table[cell], 1ull);
        else atomicAdd(&counts[cell], 1ull);
    }
    if (bad) atomicAdd(&bad_sh, bad);
    __syncthreads();
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < cells; i += kConfBlock)
            if (table[i]) atomicAdd(&counts[i], table[i]);
    }
    if (threadIdx.x == 0 && bad_sh) atomicAdd(n_bad, bad_sh);
}

template <typename S> constexpr int storage_of() { return sizeof(S) == 4 ? 1 : 0; }

template <typename S>
int launch_mn_s(const ChainDesc* descs, const EvalPart* ep, int P, int64_t n_items, int layout, const double* w,
                int d, int C1, double* tile_loss, double* tile_ok, double* classes, double* margins, int num_cus,
                hipStream_t st) {
    const bool rowlane = C1 <= kMnLaneClasses;
    const int64_t dp = mn_lds_pitch(d, storage_of<S>());
    const bool wlds = layout == kDense && (int64_t)C1 * dp <= kMnWLds;
    const int rows = layout == kDense ? kMnRows : 1;
    const int mb = rowlane ? kMnBuf : ((rows * C1 + 1) & ~1);
    const int wpad = wlds ? (int)(C1 * dp) : 0;   // (even: dp is)
    int waves = kMnWaves;
    if (!rowlane) {
        const int64_t fit = ((int64_t)kMnLdsMax - (int64_t)wpad * 8) / ((int64_t)mb * 8);
        waves = (int)(fit < 1 ? 1 : fit > kMnWaves ? kMnWaves : fit);
    }
    const size_t lds = ((size_t)wpad + (size_t)waves * mb) * sizeof(double);
    // a persistent grid: two workgroups a CU, fewer when there are fewer tiles than waves
    const int64_t want = (n_items + waves - 1) / waves;
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 2 * (kMnWaves / waves);
    const unsigned blocks = (unsigned)(want < cap ? want : cap);
    auto go = [&](auto k, auto... args) {
        (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k, dim3(blocks), dim3(waves * 64), lds, st, args...);
        return (int)hipGetLastError();
    };
    if (layout == kCsr) {
        if (rowlane) return go(score_csr_mn<S, true>, descs, ep, P, n_items, w, d, C1, mb, tile_loss, tile_ok, classes, margins);
        return go(score_csr_mn<S, false>, descs, ep, P, n_items, w, d, C1, mb, tile_loss, tile_ok, classes, margins);
    }
    if (wlds && rowlane)
        return go(score_dense_mn<S, true, true>, descs, ep, P, n_items, w, d, C1, mb, wpad, tile_loss, tile_ok, classes, margins);
    if (wlds)
        return go(score_dense_mn<S, true, false>, descs, ep, P, n_items, w, d, C1, mb, wpad, tile_loss, tile_ok, classes, margins);
    if (rowlane)
        return go(score_dense_mn<S, false, true>, descs, ep, P, n_items, w, d, C1, mb, wpad, tile_loss, tile_ok, classes, margins);
    return go(score_dense_mn<S, false, false>, descs, ep, P, n_items, w, d, C1, mb, wpad, tile_loss, tile_ok, classes, margins);
}

}  // namespace

int64_t mn_lds_pitch(int d, int storage) {
    const int vec = storage == 1 ? 4 : 2;
    return ((int64_t)d + vec - 1) / vec * vec;
}

int launch_score_mn(const ChainDesc* descs, const EvalPart* ep, int n_parts, int64_t n_items, int layout, int storage,
                    const double* w, int d, int num_classes, double* tile_loss, double* tile_ok, double* classes,
                    double* margins, int num_cus, hipStream_t st) {
    if (n_items <= 0) return 0;
    const int C1 = num_classes - 1;
    return storage == 1 ? launch_mn_s<float>(descs, ep, n_parts, n_items, layout, w, d, C1, tile_loss, tile_ok,
                                             classes, margins, num_cus, st)
                        : launch_mn_s<double>(descs, ep, n_parts, n_items, layout, w, d, C1, tile_loss, tile_ok,
                                              classes, margins, num_cus, st);
}

int launch_confusion(const double* pred, const double* lab, int64_t n, int num_classes, int64_t* counts,
                     int64_t* n_bad, int num_cus, hipStream_t st) {
    if (n <= 0) return 0;
    const int64_t want = (n + kConfBlock - 1) / kConfBlock;
    const int64_t cap = (int64_t)(num_cus > 0 ? num_cus : 256) * 4;
    const unsigned blocks = (unsigned)(want < cap ? want : cap);
    auto* c = reinterpret_cast<unsigned long long*>(counts);
    auto* b = reinterpret_cast<unsigned long long*>(n_bad);
    if ((int64_t)num_classes * num_classes <= kConfLdsCells)
        hipLaunchKernelGGL(confusion_count<true>, dim3(blocks), dim3(kConfBlock), 0, st, pred, lab, n, num_classes, c, b);
    else
        hipLaunchKernelGGL(confusion_count<false>, dim3(blocks), dim3(kConfBlock), 0, st, pred, lab, n, num_classes, c, b);
    return (int)hipGetLastError();
}

}  // namespace psgd
