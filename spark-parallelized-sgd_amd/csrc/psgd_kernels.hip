// psgd_kernels.hip -- CDNA4 (gfx950) kernels for the parallelized-SGD hot path.
//
// Reference (paths under /root/reference, src/main/scala/org/apache/spark/mllib/optimization/):
//   chain loop      ParallelizedSGD.scala:243-270   -> chain_dense_reg / chain_general
//   gradients       [ext] MLlib 1.6.1 Gradient.scala (called at ParallelizedSGD.scala:254)
//   updaters        SGDUpdater.scala:86-98, :126-148, :163-181, :199-227, :252-285
//   isConverged     ParallelizedSGD.scala:324-336 (per-sample form at :262)
//   combine         ParallelizedSGD.scala:271-276   -> fold_kernel
//
// Mapping: one wavefront64 = one chain (= one RDD partition). The chain is sequential in its
// samples; parallelism comes from the chains (one per CU) and, inside a chain, from the feature
// dimension spread over the 64 lanes. Per sample: a d-long dot reduced across the wave with
// DPP row ops + gfx950 permlane16/32 swaps (all lanes end with the bit-identical sum), the
// gradient's scalar multiplier, and the updater's elementwise update, all in registers.
// No MFMA: per-sample GEMV + axpy is not a dense contraction.
//
// Arithmetic follows the reference operator by operator (this file is compiled with
// -ffp-contract=off): grad_i = mult * x_i, then w_i = w_i + (-s) * grad_i (Breeze axpy over
// the MLlib gradient), L2 scaling w_i * (1 - s*lambda) before it. Only the dot product and the
// norms are reassociated (wave tree instead of the F2J left fold), so fp64 mode agrees with the
// reference to rounding, not bitwise.
#include "psgd_device.h"

#include "psgd_dispatch.h"

#include <stdlib.h>
#include <string.h>

namespace psgd {

template <typename S, typename T, int GRAD, int UPD, bool CONV, int NV, bool FULL>
__global__ __launch_bounds__(128) void chain_dense(ChainLaunch L, KParams kp, RingGeom geom) {
    using V = typename Vec16<S>::type;
    constexpr int VEC = Vec16<S>::N;
    constexpr int E = NV * VEC;
    constexpr int ROW_BYTES = NV * 1024;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: [header 16 B][meta ring MB x 256 B][row ring R x ROW_BYTES]
    RingHeader* hdr = reinterpret_cast<RingHeader*>(smem);
    char* meta_ring = smem + sizeof(RingHeader);
    char* ring = meta_ring + geom.meta_blocks * kMetaBlockBytes;

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int chain = blockIdx.x;
    const ChainDesc dsc = L.descs[chain];
    const int d = kp.d;
    const int64_t n = dsc.n_rows;
    const int R = geom.rows;
    const int MB = geom.meta_blocks;

    if (threadIdx.x == 0) {
        hdr->ready = 0;
        hdr->consumed = 0;
        hdr->stop = 0;
    }
    __syncthreads();

    if (wave == 1) {
        ring_loader<S, NV, FULL, 4>(L, dsc, hdr, meta_ring, ring, geom, lane);
        return;
    }

    // ---------------- compute ----------------
    // Weights and rows are held as pairs (T2) so that fp32 runs on packed VALU ops
    // (v_pk_fma/mul/add_f32: two IEEE-rounded lanes per instruction).
    using T2 = T __attribute__((ext_vector_type(2)));
    constexpr int E2 = E / 2;
    T2 w[E2];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int base = (v * 64 + lane) * VEC;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const int f = base + k;
            const double wv = as_global(L.w_in)[f < d ? f : 0];  // unconditional, clamped
            w[(v * VEC + k) / 2][(v * VEC + k) % 2] = f < d ? T(wv) : T(0);
        }
    }

    // AdaGrad / Adam status (UPD.scala:193-286) in registers beside the weights, laid out as w:
    // ua = the squared-gradient accumulator (AdaGrad) or v (Adam), ub = r (Adam). The reference
    // starts each chain's status at None (`updater.initStatus`, PSGD.scala:246): the first sample
    // takes the `None` branch.
    constexpr bool STATE_A = UPD == U_ADAGRAD || UPD == U_ADAM;
    constexpr bool STATE_B = UPD == U_ADAM;
    T2 ua[STATE_A ? E2 : 1], ub[STATE_B ? E2 : 1];
#pragma unroll
    for (int e = 0; e < (STATE_A ? E2 : 1); ++e) ua[e] = T2{T(0), T(0)};
#pragma unroll
    for (int e = 0; e < (STATE_B ? E2 : 1); ++e) ub[e] = T2{T(0), T(0)};

    // Row buffers: two register copies (ping-pong) so row t+1's LDS reads are in flight while
    // sample t computes.
    T2 xb[2][E2];
    double yb[2], sb[2];
    int meta_blk = 0;
    auto read_row = [&](auto pc, const char* src, int64_t t) __attribute__((always_inline)) {
        constexpr int p = decltype(pc)::value;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            V xv = *reinterpret_cast<const V*>(src + v * 1024 + lane * 16);
            if constexpr (!FULL) {
                // vectors past the row end were not loaded: their LDS bytes are stale
                if ((v * 64 + lane) * VEC >= dsc.ld) xv = V(0);
            }
            T tmp[VEC];
            unpack<S, T>(xv, tmp);
#pragma unroll
            for (int k = 0; k < VEC; k += 2) xb[p][(v * VEC + k) / 2] = T2{tmp[k], tmp[k + 1]};
        }
        // rows are read in order: the meta block advances every kMetaRows rows
        if (t > 0 && (t & (kMetaRows - 1)) == 0) meta_blk = (meta_blk + 1 == MB) ? 0 : meta_blk + 1;
        const f64x2 meta = *reinterpret_cast<const f64x2*>(
            meta_ring + meta_blk * kMetaBlockBytes + (int)(t & (kMetaRows - 1)) * 16);
        yb[p] = meta.x;
        sb[p] = meta.y;
    };

    unsigned ready = 0;
    bool stop = false;
    // Wait until `rows` rows have landed; false (and the watchdog flag) if the loader makes no
    // progress for kWatchdogTicks.
    auto wait_rows = [&](int64_t rows) __attribute__((always_inline)) -> bool {
        if (rows > (int64_t)ready) {
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            for (;;) {
                ready = __hip_atomic_load(&hdr->ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (rows <= (int64_t)ready) break;
                if (__builtin_amdgcn_s_memrealtime() - t0 > kWatchdogTicks) {
                    __hip_atomic_fetch_or(L.watchdog, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&hdr->stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    return false;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        return true;
    };

    double loss_sum = 0.0;
    T loss_blk = T(0);          // fp32 mode: block partial, flushed to the fp64 sum every 32 rows
    // fp64 Logistic: the per-row dots go to L.zbuf64, the losses are summed after the chain
    constexpr bool ZEXT = GRAD == G_LOGISTIC && sizeof(T) == 8;
    double* zout = ZEXT ? L.zbuf64 + (int64_t)chain * L.zstride : nullptr;
    int64_t count = 0;
    const char* slot_ptr = ring;                       // slot of row t
    const char* const ring_end = ring + R * ROW_BYTES;

    auto sample = [&](auto pc, int64_t t) __attribute__((always_inline)) {
        constexpr int p = decltype(pc)::value;
        const char* next_ptr = slot_ptr + ROW_BYTES;
        if (next_ptr == ring_end) next_ptr = ring;
        if (t + 1 < n) {   // prefetch row t+1 into the other buffer
            if (!wait_rows(t + 2)) { stop = true; return; }
            read_row(std::integral_constant<int, 1 - p>{}, next_ptr, t + 1);
        }
        const T y = T(yb[p]);
        const T s = T(sb[p]);
        const T2* x = xb[p];

        // dot(data, weights): two packed partial sums; four in the fp32 mode (shorter dependent
        // chains: the next sample's dot waits on this sample's updates)
        T2 acc;
        if constexpr (sizeof(T) == 4) {
            T2 d0 = T2{T(0), T(0)}, d1 = T2{T(0), T(0)}, d2 = T2{T(0), T(0)}, d3 = T2{T(0), T(0)};
#pragma unroll
            for (int e = 0; e < E2; e += 4) {
                d0 = __builtin_elementwise_fma(x[e], w[e], d0);
                if (e + 1 < E2) d1 = __builtin_elementwise_fma(x[e + 1], w[e + 1], d1);
                if (e + 2 < E2) d2 = __builtin_elementwise_fma(x[e + 2], w[e + 2], d2);
                if (e + 3 < E2) d3 = __builtin_elementwise_fma(x[e + 3], w[e + 3], d3);
            }
            acc = (d0 + d1) + (d2 + d3);
        } else {
            T2 acc0 = T2{T(0), T(0)}, acc1 = T2{T(0), T(0)};
#pragma unroll
            for (int e = 0; e < E2; e += 2) {
                acc0 = __builtin_elementwise_fma(x[e], w[e], acc0);
                if (e + 1 < E2) acc1 = __builtin_elementwise_fma(x[e + 1], w[e + 1], acc1);
            }
            acc = acc0 + acc1;
        }
        const T z = wave_sum_uniform(acc.x + acc.y);
        if ((t & 1) == 1 || t + 1 == n) {
            // rows <= t have been read into registers: hand their slots back to the loader
            __hip_atomic_store(&hdr->consumed, (unsigned)(t + 1), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        }

        T mult, loss;
        if constexpr (ZEXT) {
            // mult as gradient_scalar; the row's loss (log1pExp: a second exp and a log1p on
            // the sequential wave) is summed after the chain by logistic_loss64_kernel from z
            mult = (T(1) / (T(1) + m_exp(-z))) - y;
            loss = T(0);
            if (lane == 0) zout[t] = z;
        } else if constexpr (GRAD == G_LEAST_SQUARES) {
            // loss = diff*diff/2.0: the halving is exact, so the chain accumulates diff*diff and
            // halves the sum (identical to summing the halves)
            mult = z - y;
            loss = mult * mult;
        } else {
            loss = gradient_scalar<GRAD, T>(z, y, mult);
        }
        if constexpr (sizeof(T) == 4) {
            loss_blk += loss;
            if ((t & 31) == 31) { loss_sum += double(loss_blk); loss_blk = T(0); }
        } else {
            loss_sum += loss;
        }
        count += 1;

        const T a = -s;
        T2 dsq2 = T2{T(0), T(0)}, nsq2 = T2{T(0), T(0)};
        // Adam's per-sample scalars (UPD.scala:258-262): iter = j, lr = s / (1 - beta^iter)
        const bool first = t == 0;
        const T iter = T(t + 1);
        T al = T(0);
        if constexpr (UPD == U_ADAM) {
            // fp32 mode: beta^iter by the hardware log2 / exp2, as r^iter below
            if constexpr (sizeof(T) == 4) al = -(s / (T(1) - pow_fast(T(kp.beta), iter)));
            // fp64: 1 - beta^iter as 1.0 once beta^iter <= 2^-54 (bit-identical, no library pow
            // per sample on the chain) and the division by rcp + one Newton step
            else al = -(s * recip_newton(one_minus_pow_iter(T(kp.beta), iter)));
        }
#pragma unroll
        for (int e = 0; e < E2; ++e) {
            const T2 old = w[e];
            T2 nw;
            if constexpr (UPD == U_ADAGRAD) {
                // accum = None ? g*g : accum + g*g; w += -s * (g / sqrt(accum + 1.0))
                const T2 g = mult * x[e];
                const T2 acc2 = first ? g * g : ua[e] + g * g;
                ua[e] = acc2;
                if constexpr (sizeof(T) == 4) {
                    // fp32 mode: g * rsqrt(accum + 1) (one v_rsq_f32, ~1 ulp) for g / sqrt(accum + 1)
                    nw.x = old.x + a * (g.x * __builtin_amdgcn_rsqf(acc2.x + T(1)));
                    nw.y = old.y + a * (g.y * __builtin_amdgcn_rsqf(acc2.y + T(1)));
                } else {
                    // g / pow(accum + 1.0, 0.5) (UPD.scala:209) as g * rsqrt(accum + 1): v_rsq_f64
                    // and one Newton step (4.3e-15 relative, tools/newton_check; the library sqrt + division were
                    // ~20 dependent f64 operations per coordinate and sample)
                    nw.x = old.x + a * (g.x * rsqrt_newton(acc2.x + T(1)));
                    nw.y = old.y + a * (g.y * rsqrt_newton(acc2.y + T(1)));
                }
            } else if constexpr (UPD == U_ADAM) {
                // the reference's variant, literally: v = beta v + (1-beta) g,
                // r = gamma r + (1-gamma) g^2, fix1 = sqrt(1 - r^iter) + eps, w += -lr * v / fix1
                const T beta = T(kp.beta), gamma = T(kp.gamma);
                const T2 g = mult * x[e];
                const T2 sq = g * g;
                T2 v, r;
                if (first) { v = g * (T(1) - beta); r = sq * (T(1) - gamma); }
                else { v = ua[e] * beta + g * (T(1) - beta); r = ub[e] * gamma + sq * (T(1) - gamma); }
                ua[e] = v;
                ub[e] = r;
                // fp32 mode: r^iter = exp2(iter * log2 r) (v_log_f32 / v_exp_f32; r = 0 gives 0,
                // r > 1 overflows to inf and fix1 to NaN, as pow does)
                // and v / fix1 as v * rcp(fix1), sqrt by v_sqrt_f32 (~1 ulp each; a negative
                // 1 - r^iter still gives NaN)
                if constexpr (sizeof(T) == 4) {
                    const T fx = __builtin_amdgcn_sqrtf(T(1) - pow_fast(r.x, iter)) + T(kp.eps);
                    const T fy = __builtin_amdgcn_sqrtf(T(1) - pow_fast(r.y, iter)) + T(kp.eps);
                    nw.x = old.x + al * (v.x * __builtin_amdgcn_rcpf(fx));
                    nw.y = old.y + al * (v.y * __builtin_amdgcn_rcpf(fy));
                } else {
                    // sqrt and v / fix1 by the hardware estimates + one Newton step (~1e-14)
                    const T fx = sqrt_newton(one_minus_pow_iter(r.x, iter)) + T(kp.eps);
                    const T fy = sqrt_newton(one_minus_pow_iter(r.y, iter)) + T(kp.eps);
                    nw.x = old.x + al * (v.x * recip_newton(fx));
                    nw.y = old.y + al * (v.y * recip_newton(fy));
                }
            } else if constexpr (UPD == U_SQUARED_L2) {
                const T c = T(1) - s * T(kp.reg);
                nw = old * c;                       // brzWeights :*= (1 - s*lambda)
                nw = nw + a * (mult * x[e]);        // axpy(-s, grad, w)
            } else if constexpr (UPD == U_L1) {
                const T shrink = T(kp.reg) * s;
                nw = old + a * (mult * x[e]);
                nw.x = jsignum(nw.x) * jmax(T(0), m_fabs(nw.x) - shrink);
                nw.y = jsignum(nw.y) * jmax(T(0), m_fabs(nw.y) - shrink);
            } else if constexpr (sizeof(T) == 4) {
                // fp32 throughput mode: one fused update per pair, w + (-s*mult) * x
                nw = __builtin_elementwise_fma(T2{a * mult, a * mult}, x[e], old);
            } else {
                nw = old + a * (mult * x[e]);   // the reference's two roundings (fp64 mode)
            }
            w[e] = nw;
            if constexpr (CONV) { const T2 df = old - nw; dsq2 += df * df; nsq2 += nw * nw; }
        }
        slot_ptr = next_ptr;
        if constexpr (CONV) {
            T dsq = dsq2.x + dsq2.y, nsq = nsq2.x + nsq2.y;
            wave_sum2(dsq, nsq);
            // ||old - new|| < tol * max(||new||, 1.0)   (PSGD.scala:262, :333-335)
            if (m_sqrt(dsq) < T(kp.tol) * jmax(m_sqrt(nsq), T(1))) {
                __hip_atomic_store(&hdr->stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                stop = true;
            }
        }
    };

    if (n > 0) {
        if (wait_rows(1)) read_row(std::integral_constant<int, 0>{}, ring, 0);
        else stop = true;
    }
    int64_t t = 0;
    for (; t + 2 <= n && !stop; t += 2) {
        sample(std::integral_constant<int, 0>{}, t);
        if (stop) break;
        sample(std::integral_constant<int, 1>{}, t + 1);
    }
    if (t < n && !stop) sample(std::integral_constant<int, 0>{}, t);
    if constexpr (sizeof(T) == 4) loss_sum += double(loss_blk);
    if constexpr (GRAD == G_LEAST_SQUARES) loss_sum = loss_sum / 2.0;

    // regVal of the chain's last update (PSGD.scala:257; 0.0 if no sample, :247)
    double rv = 0.0;
    if constexpr (UPD == U_SQUARED_L2 || UPD == U_L1) {
        T acc = T(0);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const T we = w[e / 2][e % 2];
            if constexpr (UPD == U_SQUARED_L2) acc += we * we;
            else acc += m_fabs(we);
        }
        acc = wave_sum(acc);
        if (count > 0) {
            if constexpr (UPD == U_SQUARED_L2) {
                const double nrm = sqrt(double(acc));
                rv = 0.5 * kp.reg * nrm * nrm;
            } else {
                rv = double(acc) * kp.reg;
            }
        }
    }

    double* wo = L.w_out + (int64_t)chain * d;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int base = (v * 64 + lane) * VEC;
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (base + k < d) wo[base + k] = double(w[(v * VEC + k) / 2][(v * VEC + k) % 2]);
    }
    if (lane == 0) {
        L.rv[chain] = rv;
        if constexpr (!ZEXT) L.loss[chain] = loss_sum;
        L.cnt[chain] = count;
        L.cnt_d[chain] = double(count);
    }
}

// ------------------------------------------------------------------------------------------
// chain_general: any d, dense or CSR rows, every updater. Parity path, fp64 compute.
// The chain's working weights live in its own slice of w_out (global memory, L2-resident for
// moderate d); stateful updaters keep their status in `state`. One wave per chain.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_mem_fence() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

template <typename S, int LAYOUT, int GRAD, int UPD, bool CONV>
__global__ __launch_bounds__(64) void chain_general(ChainLaunch L, KParams kp) {
    const int lane = threadIdx.x;
    const int chain = blockIdx.x;
    const ChainDesc dsc = L.descs[chain];
    const int d = kp.d;
    const int64_t n = dsc.n_rows;
    const gptr<S> X = as_global(reinterpret_cast<const S*>(dsc.x));
    const gptr<double> Y = as_global(dsc.y);
    const gptr<double> STEPS = as_global(L.steps);
    const gptr<int64_t> ROWP = as_global(dsc.row_ptr);
    const gptr<int32_t> COL = as_global(dsc.col);
    const gmut<double> W = as_global_mut(L.w_out + (int64_t)chain * d);
    // per-chain status: dense rows [SA | SB] (2d), CSR rows [SA | SB | SC] (3d; SC: the sample's
    // dense gradient for Adam, zero outside the row's indices between samples)
    constexpr int NS = LAYOUT == kCsr ? 3 : 2;
    const gmut<double> SA = L.state ? as_global_mut(L.state + (int64_t)chain * NS * d) : nullptr;
    const gmut<double> SB = L.state ? SA + d : nullptr;
    const gmut<double> SC = (L.state && LAYOUT == kCsr) ? SA + 2 * d : nullptr;

    // CSR rows with Simple / SquaredL2 / AdaGrad and the per-sample break: ||w||^2 is carried from
    // sample to sample (O(nnz) per sample instead of a pass over all d): Simple and AdaGrad (which
    // change only the row's coordinates) add each changed coordinate's nw^2 - old^2; SquaredL2 (lazy form below) the recurrence of chain_block64,
    // ||w'||^2 = a (a ||w||^2 + 2 c z) + c^2 q, ||w - w'||^2 = b (b ||w||^2 - 2 c z) + c^2 q
    // (a = 1 - s lambda, b = 1 - a, c = -s mult, z = x . w, q = x . x). Starts from ||w_in||^2.
    constexpr bool NORMS = CONV && LAYOUT == kCsr && (UPD == U_SIMPLE || UPD == U_SQUARED_L2 || UPD == U_ADAGRAD);
    double wn = 0.0;
    for (int i = lane; i < d; i += 64) {
        const double v = as_global(L.w_in)[i];
        W[i] = v;
        if constexpr (NORMS) wn += v * v;
    }
    if constexpr (LAYOUT == kCsr && UPD == U_ADAM)
        for (int i = lane; i < d; i += 64) SC[i] = 0.0;
    wave_mem_fence();
    if constexpr (NORMS) wn = wave_sum(wn);

    // CSR rows with SquaredL2: the alpha-scaled lazy form. The chain keeps
    // w = alpha * v, so the reference's O(d) scale w *= 1 - s*lambda (UPD.scala:169) is one
    // multiply of alpha and the gradient step adds (-s g_j) / alpha to v_j at the row's indices;
    // alpha is folded back into v (O(d)) when it leaves [2^-400, 2^400] or becomes 0, and at the
    // chain's end. Equal to the reference's arithmetic up to rounding (the 1e-9 fp64 bar).
    constexpr bool LAZY = LAYOUT == kCsr && UPD == U_SQUARED_L2;
    double alpha = 1.0;
    double loss_sum = 0.0;
    int64_t count = 0;
    double rv = 0.0;
    for (int64_t t = 0; t < n; ++t) {
        const double y = Y[t];
        const double s = STEPS[t];           // stepSize / math.sqrt(iter), iter = t + 1
        gptr<S> xr = nullptr;
        int64_t kb = 0, ke = 0;
        // dot(data, weights)
        double acc = 0.0;
        [[maybe_unused]] double qacc = 0.0;   // NORMS + SquaredL2: x . x
        const int64_t ri = dsc.rows ? (int64_t)as_global(dsc.rows)[t] : t;   // sampled epoch
        if constexpr (LAYOUT == kDense) {
            xr = X + ri * dsc.ld;
            for (int i = lane; i < d; i += 64) acc = m_fma(double(xr[i]), W[i], acc);
        } else {
            kb = ROWP[ri];
            ke = ROWP[ri + 1];
            for (int64_t k = kb + lane; k < ke; k += 64) {
                acc = m_fma(double(X[k]), W[COL[k]], acc);
                if constexpr (NORMS && UPD == U_SQUARED_L2) qacc = m_fma(double(X[k]), double(X[k]), qacc);
            }
        }
        double z;
        if constexpr (NORMS && UPD == U_SQUARED_L2) {
            wave_sum2(acc, qacc);
            z = acc;
        } else {
            z = wave_sum(acc);
        }
        if constexpr (LAZY) z = alpha * z;   // dot(x, w) with w = alpha * v
        double mult;
        const double loss = gradient_scalar<GRAD, double>(z, y, mult);
        loss_sum += loss;
        count += 1;
        const double a = -s;
        double dsq = 0.0, nsq = 0.0;

        if constexpr (UPD == U_SIMPLE && LAYOUT == kCsr) {
            // Breeze axpy over the gradient's active entries only.
            for (int64_t k = kb + lane; k < ke; k += 64) {
                const int i = COL[k];
                const double old = W[i];
                const double nw = old + a * (mult * double(X[k]));
                W[i] = nw;
                if constexpr (CONV) {
                    const double df = old - nw;
                    dsq += df * df;
                    nsq += nw * nw - old * old;   // the change of ||w||^2 (NORMS)
                }
            }
        } else {
            if constexpr (LAYOUT == kCsr) {
                // Updaters that touch every coordinate: run the elementwise part over all d,
                // with the gradient applied at the row's indices in a second pass (ordered as
                // the reference: L2 scales before the axpy, L1 thresholds after it).
                if constexpr (LAZY) {
                    const double c = 1.0 - s * kp.reg;
                    if constexpr (NORMS) {
                        // ||w'||^2 and ||w - w'||^2 from the recurrence (header of this branch)
                        const double cc = a * mult, b = 1.0 - c, cq = cc * cc * qacc;
                        const double nn = c * __builtin_fma(c, wn, 2.0 * cc * z) + cq;
                        dsq = b * __builtin_fma(b, wn, -2.0 * cc * z) + cq;
                        nsq = nn > 0.0 ? nn : 0.0;
                    }
                    const double na = alpha * c;
                    if (!(__builtin_fabs(na) >= 0x1p-400 && __builtin_fabs(na) <= 0x1p400)) {
                        for (int i = lane; i < d; i += 64) W[i] = (alpha * W[i]) * c;
                        alpha = 1.0;
                        wave_mem_fence();
                    } else {
                        alpha = na;
                    }
                    for (int64_t k = kb + lane; k < ke; k += 64) {
                        const int i = COL[k];
                        W[i] = W[i] + (a * (mult * double(X[k]))) / alpha;
                    }
                } else if constexpr (UPD == U_SQUARED_L2) {
                    const double c = 1.0 - s * kp.reg;
                    for (int i = lane; i < d; i += 64) {
                        const double old = W[i];
                        const double nw = old * c;
                        W[i] = nw;
                        if constexpr (CONV) SB[i] = old;   // keep old for the convergence test
                    }
                    wave_mem_fence();
                    for (int64_t k = kb + lane; k < ke; k += 64) {
                        const int i = COL[k];
                        W[i] = W[i] + a * (mult * double(X[k]));
                    }
                } else if constexpr (UPD == U_L1) {
                    if constexpr (CONV)
                        for (int i = lane; i < d; i += 64) SB[i] = W[i];
                    wave_mem_fence();
                    for (int64_t k = kb + lane; k < ke; k += 64) {
                        const int i = COL[k];
                        W[i] = W[i] + a * (mult * double(X[k]));
                    }
                    wave_mem_fence();
                    const double shrink = kp.reg * s;
                    for (int i = lane; i < d; i += 64) {
                        const double v = W[i];
                        W[i] = jsignum(v) * jmax(0.0, fabs(v) - shrink);
                    }
                } else if constexpr (UPD == U_ADAGRAD) {
                    // UPD.scala:199-227 on a gradient that is zero outside the row's indices:
                    // the accumulator (None -> squaredGrad, i.e. zero there at the first sample)
                    // and the weights change only at the row's indices (w + a*(0/..) == w)
                    if (t == 0) {
                        for (int i = lane; i < d; i += 64) SA[i] = 0.0;
                        wave_mem_fence();
                    }
                    for (int64_t k = kb + lane; k < ke; k += 64) {
                        const int i = COL[k];
                        const double g = mult * double(X[k]);
                        const double acc2 = SA[i] + g * g;
                        SA[i] = acc2;
                        const double old = W[i];
                        const double nw = old + a * (g / sqrt(acc2 + 1.0));
                        W[i] = nw;
                        if constexpr (CONV) {
                            const double df = old - nw;
                            dsq += df * df;
                            nsq += nw * nw - old * old;   // the change of ||w||^2 (NORMS)
                        }
                    }
                } else {  // U_ADAM, UPD.scala:252-285: v and r decay at every coordinate
                    for (int64_t k = kb + lane; k < ke; k += 64) SC[COL[k]] = mult * double(X[k]);
                    wave_mem_fence();
                    const bool first = (t == 0);
                    const double beta = kp.beta, gamma = kp.gamma;
                    const double iter = double(t + 1);
                    const double lr = s / (1.0 - pow(beta, iter));
                    const double al = -lr;
                    for (int i = lane; i < d; i += 64) {
                        const double g = SC[i];
                        const double sq = g * g;
                        double v, r;
                        if (first) { v = g * (1 - beta); r = sq * (1 - gamma); }
                        else { v = SA[i] * beta + g * (1 - beta); r = SB[i] * gamma + sq * (1 - gamma); }
                        SA[i] = v;
                        SB[i] = r;
                        const double fix1 = sqrt(1.0 - pow(r, iter)) + kp.eps;
                        const double old = W[i];
                        const double nw = old + al * (v / fix1);
                        W[i] = nw;
                        if constexpr (CONV) { const double df = old - nw; dsq += df * df; nsq += nw * nw; }
                    }
                    wave_mem_fence();
                    for (int64_t k = kb + lane; k < ke; k += 64) SC[COL[k]] = 0.0;
                }
                if constexpr (CONV && UPD == U_L1) {   // (SquaredL2: the lazy form's recurrence)
                    wave_mem_fence();
                    for (int i = lane; i < d; i += 64) {
                        const double nw = W[i];
                        const double df = SB[i] - nw;
                        dsq += df * df;
                        nsq += nw * nw;
                    }
                }
            } else {
                if constexpr (UPD == U_SIMPLE) {
                    for (int i = lane; i < d; i += 64) {
                        const double old = W[i];
                        const double nw = old + a * (mult * double(xr[i]));
                        W[i] = nw;
                        if constexpr (CONV) { const double df = old - nw; dsq += df * df; nsq += nw * nw; }
                    }
                } else if constexpr (UPD == U_SQUARED_L2) {
                    const double c = 1.0 - s * kp.reg;
                    for (int i = lane; i < d; i += 64) {
                        const double old = W[i];
                        double nw = old * c;
                        nw = nw + a * (mult * double(xr[i]));
                        W[i] = nw;
                        if constexpr (CONV) { const double df = old - nw; dsq += df * df; nsq += nw * nw; }
                    }
                } else if constexpr (UPD == U_L1) {
                    const double shrink = kp.reg * s;
                    for (int i = lane; i < d; i += 64) {
                        const double old = W[i];
                        double nw = old + a * (mult * double(xr[i]));
                        nw = jsignum(nw) * jmax(0.0, fabs(nw) - shrink);
                        W[i] = nw;
                        if constexpr (CONV) { const double df = old - nw; dsq += df * df; nsq += nw * nw; }
                    }
                } else if constexpr (UPD == U_ADAGRAD) {
                    // accum = (first ? g*g : accum + g*g); w += -s * (g / sqrt(accum + 1.0))
                    const bool first = (t == 0);
                    for (int i = lane; i < d; i += 64) {
                        const double g = mult * double(xr[i]);
                        const double sq = g * g;
                        const double acc2 = first ? sq : SA[i] + sq;
                        SA[i] = acc2;
                        const double old = W[i];
                        const double nw = old + a * (g / sqrt(acc2 + 1.0));
                        W[i] = nw;
                        if constexpr (CONV) { const double df = old - nw; dsq += df * df; nsq += nw * nw; }
                    }
                } else {  // U_ADAM, UPD.scala:252-285 (reproduced literally)
                    const bool first = (t == 0);
                    const double beta = kp.beta, gamma = kp.gamma;
                    const double iter = double(t + 1);
                    const double lr = s / (1.0 - pow(beta, iter));
                    const double al = -lr;
                    for (int i = lane; i < d; i += 64) {
                        const double g = mult * double(xr[i]);
                        const double sq = g * g;
                        double v, r;
                        if (first) { v = g * (1 - beta); r = sq * (1 - gamma); }
                        else { v = SA[i] * beta + g * (1 - beta); r = SB[i] * gamma + sq * (1 - gamma); }
                        SA[i] = v;
                        SB[i] = r;
                        const double fix1 = sqrt(1.0 - pow(r, iter)) + kp.eps;
                        const double old = W[i];
                        const double nw = old + al * (v / fix1);
                        W[i] = nw;
                        if constexpr (CONV) { const double df = old - nw; dsq += df * df; nsq += nw * nw; }
                    }
                }
            }
        }
        wave_mem_fence();
        if constexpr (NORMS && UPD == U_SQUARED_L2) {
            // dsq and nsq are the recurrence's (wave-uniform)
            wn = nsq;
            if (sqrt(dsq > 0.0 ? dsq : 0.0) < kp.tol * jmax(sqrt(nsq), 1.0)) break;
        } else if constexpr (NORMS) {
            wave_sum2(dsq, nsq);
            wn = wn + nsq;
            if (sqrt(dsq) < kp.tol * jmax(sqrt(wn), 1.0)) break;
        } else if constexpr (CONV) {
            wave_sum2(dsq, nsq);
            if (sqrt(dsq) < kp.tol * jmax(sqrt(nsq), 1.0)) break;
        }
    }

    if constexpr (LAZY) {
        for (int i = lane; i < d; i += 64) W[i] = alpha * W[i];
        wave_mem_fence();
    }
    if constexpr (UPD == U_SQUARED_L2 || UPD == U_L1) {
        double acc = 0.0;
        for (int i = lane; i < d; i += 64) acc += (UPD == U_SQUARED_L2) ? W[i] * W[i] : fabs(W[i]);
        acc = wave_sum(acc);
        if (count > 0) {
            if constexpr (UPD == U_SQUARED_L2) {
                const double nrm = sqrt(acc);
                rv = 0.5 * kp.reg * nrm * nrm;
            } else {
                rv = acc * kp.reg;
            }
        }
    }
    if (lane == 0) {
        L.rv[chain] = rv;
        L.loss[chain] = loss_sum;
        L.cnt[chain] = count;
        L.cnt_d[chain] = double(count);
    }
}

// ------------------------------------------------------------------------------------------
// The reference combiner (PSGD.scala:271-276) as a left fold over n items in index order, one
// thread per coordinate; the thread with i == d folds the scalars.
//   w = (w1*c1 + w2*c2) / (c1 + c2);  rv likewise;  loss = l1 + l2;  c = c1 + c2
// out[0..d) = w, out[d] = regVal, out[d+1] = lossSum, out[d+2] = count.
//
// Each step is one dependent f64 multiply, add and IEEE division on the coordinate's running
// value; the item loads are not on that chain. Loading item p at its step (before round 6)
// left the steps waiting on memory round trips: 40 us per c2 epoch (256 chains, d = 512). The
// block stages the per-item scalars (counts, and regVal, loss, alpha as needed) in LDS,
// kFoldStage items at a time, and every coordinate thread keeps its next kFoldAhead weights in
// flight while it folds the current ones. Same operations in the same order: bit-identical
// results. (Measured and not kept: the division with its denominator-only part -- the refined
// reciprocal of c1 + c2 -- taken off the running value's dependent path, bit-identical by
// construction where v_div_scale scales nothing and checked over the whole f64 range: 33 us
// against 28 per c2 epoch, the extra reciprocal work per step costs more than the shorter path.)
// ------------------------------------------------------------------------------------------
constexpr int kFoldStage = 512;    // items staged in LDS at a time
constexpr int kFoldAhead = 16;     // weight loads in flight per coordinate thread
constexpr int kFoldThreads = 256;

// WLOAD(p, a) -> item p's weight for this thread's coordinate (a = item p's alpha, if staged)
template <bool ALPHA, typename WLoad>
__device__ __forceinline__ void fold_items(WLoad wload, const double* __restrict__ alpha,
                                           const double* __restrict__ rv, const double* __restrict__ loss,
                                           const double* __restrict__ cnt, int64_t s_stride, int n, int d,
                                           double* __restrict__ out, int* __restrict__ watchdog,
                                           double* __restrict__ mirror) {
    __shared__ double sc[kFoldStage], sr[kFoldStage], sl[kFoldStage], sa[ALPHA ? kFoldStage : 1];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool wt = i < d;                                   // a weight coordinate
    const bool st = i == d;                                  // the scalars
    const bool blk_st = (int)(blockIdx.x * blockDim.x) <= d && d < (int)((blockIdx.x + 1) * blockDim.x);
    double acc = 0.0, r = 0.0, l = 0.0, c1 = 0.0;
    for (int s0 = 0; s0 < n; s0 += kFoldStage) {
        const int m = n - s0 < kFoldStage ? n - s0 : kFoldStage;
        __syncthreads();   // the previous stage's items are folded
        for (int k = threadIdx.x; k < m; k += blockDim.x) {
            const int64_t q = (int64_t)(s0 + k) * s_stride;
            sc[k] = cnt[q];
            if (blk_st) {
                sr[k] = rv[q];
                sl[k] = loss[q];
            }
            if constexpr (ALPHA) sa[k] = alpha[s0 + k];
        }
        __syncthreads();
        const int k0 = s0 == 0 ? 1 : 0;   // item 0 starts the fold
        if (s0 == 0) {
            c1 = sc[0];
            if (wt) acc = wload(0, ALPHA ? sa[0] : 1.0);
            if (st) {
                r = sr[0];
                l = sl[0];
            }
        }
        if (wt) {
            // items [k0, m) of the stage, kFoldAhead at a time, the next group's loads issued
            // before the current group's steps (indices clamped to the stage: a group past its
            // end loads item m - 1 again and folds nothing)
            double cur[kFoldAhead], nxt[kFoldAhead];
            auto fetch = [&](double (&v)[kFoldAhead], int g0) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < kFoldAhead; ++j) {
                    const int k = g0 + j < m ? g0 + j : m - 1;
                    v[j] = wload(s0 + k, ALPHA ? sa[k] : 1.0);
                }
            };
            fetch(cur, k0);
            for (int g0 = k0; g0 < m; g0 += kFoldAhead) {
                fetch(nxt, g0 + kFoldAhead);
#pragma unroll
                for (int j = 0; j < kFoldAhead; ++j) {
                    if (g0 + j < m) {
                        const double c2 = sc[g0 + j];
                        acc = (acc * c1 + cur[j] * c2) / (c1 + c2);
                        c1 = c1 + c2;
                    }
                }
#pragma unroll
                for (int j = 0; j < kFoldAhead; ++j) cur[j] = nxt[j];
            }
        } else if (st) {
            for (int k = k0; k < m; ++k) {
                const double c2 = sc[k];
                r = (r * c1 + sr[k] * c2) / (c1 + c2);
                l = l + sl[k];
                c1 = c1 + c2;
            }
        }
    }
    if (wt) {
        out[i] = acc;
    } else if (st) {
        // a chain kernel that tripped its watchdog poisons the count: the host raises. The
        // flags are cleared here for the next epoch (every epoch's chains end in one fold), so
        // the epoch enqueues no memset of its own
        bool fired = false;
        if (watchdog) {
            fired = watchdog[0] != 0;   // (the chains' flags are OR-ed into word 0)
            watchdog[0] = watchdog[1] = watchdog[2] = watchdog[3] = 0;
        }
        const double cnt_out = fired ? __builtin_nan("") : c1;
        out[d] = r;
        out[d + 1] = l;
        out[d + 2] = cnt_out;
        if (mirror) {
            // the host's copy, system-scope stores; the count last, with release order, so a
            // host that polls it (for a value other than the one it left there) then reads the
            // other two finds them written
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(mirror), (unsigned long long)__double_as_longlong(r),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(mirror) + 1, (unsigned long long)__double_as_longlong(l),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(mirror) + 2,
                               (unsigned long long)__double_as_longlong(cnt_out), __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

__global__ __launch_bounds__(kFoldThreads) void fold_kernel(const double* __restrict__ w, int64_t w_stride,
                            const double* __restrict__ rv, const double* __restrict__ loss,
                            const double* __restrict__ cnt, int64_t s_stride, int n, int d,
                            double* __restrict__ out, int* __restrict__ watchdog, double* __restrict__ mirror) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    fold_items<false>([&](int p, double) { return w[(int64_t)p * w_stride + i]; }, nullptr, rv, loss, cnt,
                      s_stride, n, d, out, watchdog, mirror);
}

// The same combiner over the fp32 CSR chains' weights, w_p = walpha[p] * double(v_p[i]) -- the
// value those chains once wrote to w_out, so the fold's arithmetic is unchanged; reading the
// fp32 vectors directly saves the O(P d) f64 write and re-read (C5: 2^22 features x 1024 chains).
// (V = double: chain_sparse64's vectors, the same combiner with w_p = walpha[p] * v_p[i] -- the
// value chain_general's W[i] = alpha * W[i] writes at the chain's end.)
template <typename V>
__global__ __launch_bounds__(kFoldThreads) void fold_scaled_kernel(const V* __restrict__ v, int64_t v_stride,
                                const double* __restrict__ alpha, const double* __restrict__ rv,
                                const double* __restrict__ loss, const double* __restrict__ cnt,
                                int n, int d, double* __restrict__ out, int* __restrict__ watchdog,
                                double* __restrict__ mirror) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    fold_items<true>([&](int p, double a) { return a * double(v[(int64_t)p * v_stride + i]); }, alpha, rv, loss,
                     cnt, 1, n, d, out, watchdog, mirror);
}

int launch_fold_f32(const float* wf32, int64_t wstride, const double* walpha, const double* rv,
                    const double* loss, const double* cnt, int n, int d, double* out,
                    int* watchdog, hipStream_t stream, double* mirror) {
    if (n <= 0) return -1;
    const int threads = kFoldThreads;
    const int blocks = (d + 1 + threads - 1) / threads;
    hipLaunchKernelGGL(fold_scaled_kernel<float>, dim3(blocks), dim3(threads), 0, stream, wf32, wstride, walpha,
                       rv, loss, cnt, n, d, out, watchdog, mirror);
    return (int)hipGetLastError();
}

int launch_fold_f64(const double* wv, int64_t wstride_d, const double* walpha, const double* rv,
                    const double* loss, const double* cnt, int n, int d, double* out,
                    int* watchdog, hipStream_t stream, double* mirror) {
    if (n <= 0) return -1;
    const int threads = kFoldThreads;
    const int blocks = (d + 1 + threads - 1) / threads;
    hipLaunchKernelGGL(fold_scaled_kernel<double>, dim3(blocks), dim3(threads), 0, stream, wv, wstride_d, walpha,
                       rv, loss, cnt, n, d, out, watchdog, mirror);
    return (int)hipGetLastError();
}

// sum((a-b)^2) and sum(b^2) (a may be null: then sum(b^2) and sum(|b|)) -- one block, fixed
// reduction tree, deterministic.
__global__ __launch_bounds__(256) void sq_terms_kernel(const double* __restrict__ a,
                                                       const double* __restrict__ b, int d,
                                                       double* __restrict__ out) {
    __shared__ double s0[256], s1[256];
    double t0 = 0.0, t1 = 0.0;
    for (int i = threadIdx.x; i < d; i += 256) {
        const double bv = b[i];
        if (a) { const double df = a[i] - bv; t0 += df * df; t1 += bv * bv; }
        else { t0 += bv * bv; t1 += fabs(bv); }
    }
    s0[threadIdx.x] = t0;
    s1[threadIdx.x] = t1;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            s0[threadIdx.x] += s0[threadIdx.x + h];
            s1[threadIdx.x] += s1[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = s0[0]; out[1] = s1[0]; }
}

// The fp64 Logistic chain's lossSum (PSGD.scala:254/:259; [ext] MLlib 1.6.1 LogisticGradient:
// margin = -z, loss = y > 0 ? log1pExp(margin) : log1pExp(margin) - margin) from the dots z_t
// chain_dense stored, one 1024-thread workgroup per chain. Every row's loss is the reference's
// arithmetic on the chain's own z_t; only the sum is a tree instead of the sequential `+=`
// (within the fp64 1e-9 bar).
__global__ __launch_bounds__(1024) void logistic_loss64_kernel(ChainLaunch L) {
    const int chain = blockIdx.x;
    const int64_t n = L.cnt[chain];
    const double* y = L.descs[chain].y;
    const double* z = L.zbuf64 + (int64_t)chain * L.zstride;
    double acc = 0.0;
    for (int64_t t = threadIdx.x; t < n; t += blockDim.x) {
        double mult;
        acc += gradient_scalar<G_LOGISTIC, double>(as_global(z)[t], as_global(y)[t], mult);
    }
    acc = wave_sum(acc);
    __shared__ double part[16];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < 16; ++k) s += part[k];
        L.loss[chain] = s;
    }
}

// stepSize / math.sqrt(iter) for iter = 1..n (SGDUpdater.scala:93, :133, :174, :210, :261).
__global__ void steps_kernel(double step, int64_t n, double* __restrict__ steps) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) steps[j] = step / sqrt(double(j + 1));
}

// ------------------------------------------------------------------------------------------
// Launchers / dispatch.
// ------------------------------------------------------------------------------------------
// chain_dense's ring: the header, then the meta and row rings; at least PUB + 2 = 6 rows.
RingPlan dense_ring_plan(int nv, size_t budget) {
    return plan_ring(budget, sizeof(RingHeader), nv, 0, 1, 6);
}

int ring_geometry(int family, int nv, int compute, bool conv, int64_t budget, int32_t* out5) {
    if (!out5 || (nv != 1 && nv != 2 && nv != 4 && nv != 8)) return -1;
    const size_t b = budget > 0 ? (size_t)budget : (size_t)64 * 1024;   // as the launchers
    RingPlan p;
    switch (family) {
    case kRingDense: p = dense_ring_plan(nv, b); break;
    case kRingSplit:
        if (nv < 2) return -1;
        p = split_ring_plan(nv, compute, conv, b);
        break;
    case kRingBlock: p = block_ring_plan(nv, conv, b); break;
    case kRingBlock64: p = block64_ring_plan(nv, conv, b); break;
    default: return -1;
    }
    note_ring(out5, p.g);
    out5[4] = (int32_t)p.bytes;
    return 0;
}

int launch_logistic_loss64(const ChainLaunch& L, int n_chains, hipStream_t st) {
    if (!L.zbuf64) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(logistic_loss64_kernel, dim3(n_chains), dim3(1024), 0, st, L);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// plan_chains: which kernel runs the epoch and what it needs, decided once, on the
// host. The environment switches of the selection are read here and nowhere else: every call
// reads them (the tests set them between epochs), but for PSGD_B64_WAVES and PSGD_SPLIT, which
// are read once per process: by the first plan that reaches their clause, psgd_plan_chains
// included, so a test that wants them sets them before the first plan of its process.
// ------------------------------------------------------------------------------------------
namespace {

const char* env_or_empty(const char* name) {
    const char* e = getenv(name);
    return e ? e : "";
}

void plan_ring_of(ChainPlan& p, const RingPlan& r) {
    note_ring(p.ring, r.g);
    p.lds_bytes = (int64_t)r.bytes;
}

// chain_sparse_lds at the depth PSGD_SPARSE_SK asks for (`depth`), in the arithmetic of
// spec.compute. Whether it applies is decided at `depth`; the per-sample break has instances at
// SK = 4 only. PSGD_SPARSE_LDS_HEAD=k caps the LDS-resident head (tests of the tail at small d).
bool plan_sparse_lds(ChainPlan& p, int depth) {
    const ChainSpec& s = p.spec;
    if (s.max_nnz > sparse_lds_row_cap() || s.n_max > (int64_t)INT32_MAX) return false;
    if (sparse_lds_head(depth, s.compute, s.d) < 0) return false;
    p.family = kFamSparseLds;
    p.sk = depth == 8 && !s.conv ? 8 : 4;
    p.lds_k = sparse_lds_head(p.sk, s.compute, s.d);
    const char* e = env_or_empty("PSGD_SPARSE_LDS_HEAD");
    if (*e) {
        const int64_t cap = atoll(e) & ~int64_t(3);
        if (cap >= 0 && cap < p.lds_k) p.lds_k = cap;
    }
    p.tail = p.lds_k < s.d;
    p.lds_bytes = sparse_lds_bytes(p.sk, s.compute, s.d, p.lds_k);
    p.variant = 600 + (s.conv ? 40 : 0) + (p.sk == 8 ? 10 : 0) + (s.compute == 0 ? 20 : 0) + s.storage;
    return true;
}

}  // namespace

ChainPlan plan_chains(const ChainSpec& s) {
    ChainPlan p{};
    p.spec = s;
    p.conv = s.conv;
    p.weights_in = kWeightsOut;
    const bool dense = s.layout == kDense, csr = !dense, f32c = s.compute == 1;
    const bool logistic = s.gradient == G_LOGISTIC;
    const bool simple_l2 = s.updater == U_SIMPLE || s.updater == U_SQUARED_L2;
    const int vec = s.storage == 1 ? 4 : 2;
    const size_t budget = s.lds_budget > 0 ? (size_t)s.lds_budget : (size_t)64 * 1024;
    // the rows' margins (fp32) / dots (fp64) of a dense binary Logistic epoch: its loss is summed
    // after the chain by the kernels that leave them there
    if (dense && logistic) p.zbuf = f32c ? kBufF32 : s.nc == 0 ? kBufF64 : kBufNone;
    if (s.nc > 0) {   // LogisticGradient(numClasses > 2)
        p.family = kFamMultinomial;
        p.variant = 500 + s.layout;
        p.lds_bytes = 2 * (int64_t)s.nc * (int64_t)sizeof(double);
        return p;
    }
    if (dense) {
        p.nv = 1;
        while ((int64_t)p.nv * 64 * vec < s.max_ld) p.nv *= 2;
        // FULL: every lane's every vector is inside every row (no exec masking on the loads)
        p.full = s.min_ld >= (int64_t)p.nv * 64 * vec;
    }
    // a chain's vector of the CSR throughput kernels: d floats / doubles, and 128 + 1024 the
    // kernels' masked-off lanes load from / store to (256-byte aligned: the set-up stores 16-byte
    // vectors). PSGD_SPARSE_SK=8: chain_sparse_lds speculates 8 rows deep (A/B measurements).
    const int64_t vstride = ((int64_t)s.d + 128 + 1024 + 63) / 64 * 64;
    const int depth = csr && atoi(env_or_empty("PSGD_SPARSE_SK")) == 8 ? 8 : 4;
    auto want_vectors = [&](int buf) {
        p.vec = buf;
        p.vec_stride = buf == kBufF64 ? 2 * vstride : vstride;
        p.walpha = p.wnsq0_buf = true;
        // (the fp32 LDS head of chain_sparse_lds, below which the chains never touch the vector;
        // the fp64 head is shorter: half of it is inside the fp64 tail)
        const int64_t head = sparse_lds_head(depth, 1, s.d);
        p.reroll_head = head > 0 ? head : 0;
    };
    // every fp32-compute CSR epoch gets its vectors, whichever kernel runs
    if (csr && f32c) want_vectors(kBufF32);

    // PSGD_PER_SAMPLE=1 keeps the per-sample kernels (A/B measurements, tests)
    const char* ps = env_or_empty("PSGD_PER_SAMPLE");
    const bool throughput = !(*ps && *ps != '0');
    // PSGD_SPARSE_KERNEL = lds | spec | plain forces an fp32 CSR kernel (any other non-empty value
    // is `plain`); hbm64 keeps fp64 CSR epochs off the LDS kernel (tests, A/B measurements)
    const char* force = env_or_empty("PSGD_SPARSE_KERNEL");

    // The 8-row Gram-block kernels: dense rows, Simple / SquaredL2, rows of up to 8 KiB, any tol
    // (PSGD_B64_CONV=0 sends tol > 0 to the per-sample kernels instead: tests of chain_split's
    // break path, A/B measurements)
    if (throughput && dense && simple_l2 && s.max_ld <= 8 * 64 * vec &&
        !(s.conv && env_or_empty("PSGD_B64_CONV")[0] == '0')) {
        if (f32c) {
            p.family = kFamBlock;
            p.variant = 300 + (s.conv ? 40 : 0) + p.nv;
            plan_ring_of(p, block_ring_plan(p.nv, s.conv, budget));
            p.after = logistic ? kAfterMarginLoss : kAfterNone;
            return p;
        }
        // two chain waves from NV = 2 on; PSGD_B64_WAVES=1 keeps one where its share of a block
        // fits the registers (NV <= 4; A/B measurements)
        static const bool one_wave = atoi(env_or_empty("PSGD_B64_WAVES")) == 1;
        p.family = kFamBlock64;
        p.h = (p.nv >= 2 && !(one_wave && p.nv <= 4)) ? 2 : 1;
        p.variant = 700 + (s.conv ? 40 : 0) + 10 * (p.h - 1) + p.nv;
        plan_ring_of(p, block64_ring_plan(p.nv, s.conv, budget));
        p.after = logistic ? kAfterLogisticLoss64 : kAfterNone;
        return p;
    }
    // The fp32 CSR kernels, weights as fp32 vectors w = walpha v: in LDS (rows of <= 128 non-zeros,
    // d up to ~65k), else speculating from HBM (no per-sample break), else plain
    if (throughput && csr && f32c && simple_l2) {
        p.weights_in = kWeightsF32;
        p.setup = kSetupWf32;
        p.wnsq0 = s.updater == U_SQUARED_L2 || s.conv ? kWnsq0Rounded : kWnsq0None;
        const bool no_lds = *force && strcmp(force, "lds") != 0;
        const bool no_spec = *force && strcmp(force, "spec") != 0;
        if (!no_lds && plan_sparse_lds(p, depth)) return p;
        const int64_t spec_bytes = sparse_spec_bytes(s.d, s.max_nnz);
        if (!no_spec && !s.conv && spec_bytes >= 0) {
            p.family = kFamSparseSpec;
            p.variant = 410 + s.storage;
            p.sk = 8;
            p.lds_bytes = spec_bytes;
            return p;
        }
        p.family = kFamSparse;
        p.variant = 400 + (s.conv ? 40 : 0) + s.storage;
        return p;
    }
    // The fp64 CSR kernels: Simple, and SquaredL2 while alpha stays in range; the chain's f64
    // vector in LDS with its tail in HBM (weights end in w_out), or beyond that kernel's range
    // all of it in HBM (w = walpha v). Without the vectors the epoch runs chain_general.
    if (throughput && csr && !f32c && !s.f64_vectors_unavailable &&
        (s.updater == U_SIMPLE || (s.updater == U_SQUARED_L2 && s.alpha_ok))) {
        want_vectors(kBufF64);
        p.wnsq0 = s.conv ? kWnsq0Exact : kWnsq0None;   // ||w_in||^2 for the break's norm recurrence
        if (strcmp(force, "hbm64") != 0 && plan_sparse_lds(p, depth)) return p;
        p.family = kFamSparse64;
        p.variant = 420 + (s.conv ? 40 : 0) + s.storage;
        p.weights_in = kWeightsF64;
        p.setup = kSetupW64;
        return p;
    }
    // The feature-split per-sample chain: dense rows of 2 .. 8 KiB; AdaGrad / Adam / L1 always,
    // Simple / SquaredL2 with the per-sample break that the blocked kernels did not take.
    // PSGD_SPLIT=0 keeps chain_dense (A/B measurements)
    static const bool split_off = env_or_empty("PSGD_SPLIT")[0] == '0';
    if (throughput && dense && (!simple_l2 || s.conv) && !split_off && p.nv >= 2 && p.nv <= 8) {
        p.family = kFamSplit;
        p.h = split_waves(p.nv);
        p.variant = 800 + 10 * p.h + p.nv;
        plan_ring_of(p, split_ring_plan(p.nv, s.compute, s.conv, budget));
        p.after = !logistic ? kAfterNone : f32c ? kAfterMarginLoss : kAfterLogisticLoss64;
        return p;
    }
    // chain_dense, weights (and AdaGrad / Adam status) in registers: up to 8 row vectors per lane;
    // fp64 AdaGrad / Adam up to 16 doubles per lane (weights, status and two row buffers are 5 x
    // 16 doubles = 160 VGPRs), d <= 1,024
    const bool wide_state = s.updater >= U_ADAGRAD && !f32c;
    if (dense && s.max_ld <= (wide_state ? 16 * 64 : 8 * 64 * vec)) {
        p.family = kFamDense;
        p.variant = 100 + p.nv;
        plan_ring_of(p, dense_ring_plan(p.nv, budget));
        p.after = logistic && !f32c ? kAfterLogisticLoss64 : kAfterNone;
        return p;
    }
    // chain_general: any row, weights in w_out and status in HBM
    p.family = kFamGeneral;
    p.variant = 200 + s.layout;
    p.nv = 0;
    p.full = false;
    return p;
}

extern "C" int32_t psgd_plan_chains(const int64_t* spec, int32_t n_spec, int64_t* plan, int32_t n_plan) {
    if (!spec || !plan || n_spec < 15 || n_plan < 24) return -1;
    ChainSpec s{};
    s.layout = (int32_t)spec[0];
    s.storage = (int32_t)spec[1];
    s.compute = (int32_t)spec[2];
    s.gradient = (int32_t)spec[3];
    s.updater = (int32_t)spec[4];
    s.conv = spec[5] != 0;
    s.d = (int32_t)spec[6];
    s.nc = (int32_t)spec[7];
    s.min_ld = spec[8];
    s.max_ld = spec[9];
    s.max_nnz = spec[10];
    s.n_max = spec[11];
    s.alpha_ok = spec[12] != 0;
    s.lds_budget = spec[13];
    s.f64_vectors_unavailable = spec[14] != 0;
    const ChainPlan p = plan_chains(s);
    const int64_t out[24] = {p.family, p.variant, p.nv, p.h, p.full, p.conv, p.sk, p.lds_k, p.tail,
                             p.lds_bytes, p.ring[0], p.ring[1], p.ring[2], p.ring[3], p.weights_in,
                             p.after, p.setup, p.wnsq0, p.zbuf, p.vec, p.vec_stride, p.walpha,
                             p.wnsq0_buf, p.reroll_head};
    for (int k = 0; k < 24; ++k) plan[k] = out[k];
    return 0;
}

// ------------------------------------------------------------------------------------------
// Launchers: the plan's fields to the template instance (psgd_dispatch.h; the lists are the
// built instances).
// ------------------------------------------------------------------------------------------
// chain_dense and chain_general, this file's two families, share one nest.
static int launch_per_sample(const ChainLaunch& L, const KParams& kp, const ChainPlan& p, hipStream_t st) {
    const ChainSpec& s = p.spec;
    const bool dense = p.family == kFamDense;
    if (dense && p.after == kAfterLogisticLoss64 && !L.zbuf64) return (int)hipErrorInvalidValue;
    // chain_dense's ring, from the per-workgroup LDS budget (chosen by the host so that the chains
    // spread evenly over the CUs); the consumer reads rows t and t+1, the loader keeps
    // loader_depth rows in flight and drains before it blocks on a full ring.
    const RingGeom g = ring_of_plan(p).g;
    const size_t bytes = (size_t)p.lds_bytes;
    const int rc = dispatch_int<1, 0>(s.storage, [&](auto sc) {
    return dispatch_int<G_LOGISTIC, G_LEAST_SQUARES, G_HINGE>(s.gradient, [&](auto gc) {
    return dispatch_int<U_SIMPLE, U_SQUARED_L2, U_L1, U_ADAGRAD, U_ADAM>(s.updater, [&](auto uc) {
    return dispatch_bool(p.conv, [&](auto conv) {
        using S = FloatOf<decltype(sc)::value>;
        constexpr int GRAD = decltype(gc)::value, UPD = decltype(uc)::value;
        constexpr bool CONV = decltype(conv)::value;
        if (dense)
            return dispatch_int<1, 0>(s.compute, [&](auto cc) {
                using T = FloatOf<decltype(cc)::value>;
                auto launch = [&](auto nv) {
                    return dispatch_bool(p.full, [&](auto full) {
                        auto k = chain_dense<S, T, GRAD, UPD, CONV, decltype(nv)::value, decltype(full)::value>;
                        (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
                        hipLaunchKernelGGL(k, dim3(kp.n_chains), dim3(128), bytes, st, L, kp, g);
                        return (int)hipGetLastError();
                    });
                };
                // fp64 AdaGrad / Adam hold at most 16 doubles per lane: no NV = 8 on f32 rows
                if constexpr (sizeof(T) == 8 && UPD >= U_ADAGRAD && sizeof(S) == 4)
                    return dispatch_int<1, 2, 4>(p.nv, launch);
                else
                    return dispatch_int<1, 2, 4, 8>(p.nv, launch);
            });
        return dispatch_int<kDense, kCsr>(s.layout, [&](auto layout) {
            hipLaunchKernelGGL((chain_general<S, decltype(layout)::value, GRAD, UPD, CONV>), dim3(kp.n_chains),
                               dim3(64), 0, st, L, kp);
            return (int)hipGetLastError();
        });
    }); }); }); });
    if (rc || !dense || p.after != kAfterLogisticLoss64) return rc;
    return launch_logistic_loss64(L, kp.n_chains, st);
}

int launch_chains(const ChainLaunch& L, const KParams& kp, const ChainPlan& plan, hipStream_t stream) {
    if (kp.n_chains <= 0) return 0;
    switch (plan.family) {
    case kFamDense:
    case kFamGeneral: return launch_per_sample(L, kp, plan, stream);
    case kFamBlock: return launch_block(L, kp, plan, stream);
    case kFamBlock64: return launch_block64(L, kp, plan, stream);
    case kFamSplit: return launch_split(L, kp, plan, stream);
    case kFamSparse:
    case kFamSparseSpec:
    case kFamSparse64: return launch_sparse(L, kp, plan, stream);
    case kFamSparseLds: return launch_sparse_lds(L, kp, plan, stream);
    case kFamMultinomial: return launch_multinomial(L, kp, plan, stream);
    default: return (int)hipErrorInvalidValue;
    }
}

int launch_fold(const double* w, int64_t w_stride, const double* rv, const double* loss,
                const double* cnt, int64_t s_stride, int n, int d, double* out,
                int* watchdog, hipStream_t stream, double* mirror) {
    if (n <= 0) return -1;
    const int threads = kFoldThreads;
    const int blocks = (d + 1 + threads - 1) / threads;
    hipLaunchKernelGGL(fold_kernel, dim3(blocks), dim3(threads), 0, stream, w, w_stride, rv, loss,
                       cnt, s_stride, n, d, out, watchdog, mirror);
    return (int)hipGetLastError();
}

int launch_sq_terms(const double* a, const double* b, int d, double* out2, hipStream_t stream) {
    hipLaunchKernelGGL(sq_terms_kernel, dim3(1), dim3(256), 0, stream, a, b, d, out2);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Bernoulli sampling of one epoch's batch ([ext] Spark 1.6.1 BernoulliSampler on an
// XORShiftRandom, restated in oracle/psgd_oracle.c or_sample_partition). fraction <= 0.4:
// GapSamplingIterator (geometric skips, u = max(nextDouble, 5e-11), k = (int)(log(u) /
// log1p(-f)), a skip before the first row and after every returned row); else the filter
// nextDouble() <= fraction per row, in iterator order.
//
// The reference walks one XORShift sequence per partition; a lane doing the same is bound by
// one dependent label load per row (~20 ms for 40k-row partitions). Both samplers consume
// exactly two XORShift steps per draw (one nextDouble), and XORShift is linear over GF(2), so
// draw j's state is D^j s0 with D the 64x64 bit matrix of two steps. One workgroup per
// partition: thread i owns draws [r + 64 i, r + 64 i + 64) of round r (16384 draws a round),
// reaching its first state through the jump matrices D^(64 * 2^k) (built at compile time),
// and an exclusive scan over threads places its output: the filter's kept-row counts, or
// the gap sampler's positions (pos_j = sum_{i<=j} k_i + j, strictly increasing, so the
// emitted rows are exactly the draws with pos_j < n_rows and row j lands at index j).
// ------------------------------------------------------------------------------------------
namespace {
struct Gf2Mat {
    uint64_t c[64];   // column b = D * e_b
};
constexpr uint64_t xs_step(uint64_t x) {
    x ^= x << 21;
    x ^= x >> 35;
    x ^= x << 4;
    return x;
}
constexpr uint64_t gf2_apply_c(const Gf2Mat& m, uint64_t s) {
    uint64_t r = 0;
    for (int b = 0; b < 64; ++b)
        if ((s >> b) & 1) r ^= m.c[b];
    return r;
}
constexpr Gf2Mat gf2_square(const Gf2Mat& m) {
    Gf2Mat r{};
    for (int b = 0; b < 64; ++b) r.c[b] = gf2_apply_c(m, m.c[b]);
    return r;
}
constexpr int kSampThreads = 256;
constexpr int kSampDraws = 64;   // draws per thread per round (a power of two: D^64 by squaring)
struct SampleJumps {
    Gf2Mat j[9];   // j[k] = D^(64 * 2^k): k < 8 place thread i, j[8] advances a round
};
constexpr SampleJumps make_sample_jumps() {
    Gf2Mat d{};
    for (int b = 0; b < 64; ++b) d.c[b] = xs_step(xs_step(1ull << b));
    for (int i = 0; i < 6; ++i) d = gf2_square(d);
    SampleJumps s{};
    s.j[0] = d;
    for (int k = 1; k < 9; ++k) s.j[k] = gf2_square(s.j[k - 1]);
    return s;
}
static_assert(kSampThreads == 256 && kSampDraws == 64, "jump table is built for 256 x 64 draws");
}  // namespace

__constant__ SampleJumps kSampleJumps = make_sample_jumps();

__device__ __forceinline__ uint64_t gf2_apply(const Gf2Mat& m, uint64_t s) {
    uint64_t r = 0;
#pragma unroll 16
    for (int b = 0; b < 64; ++b) r ^= m.c[b] & (0ull - ((s >> b) & 1));
    return r;
}

__device__ __forceinline__ int32_t xs_next(uint64_t& st, int bits) {
    const uint64_t x = xs_step(st);
    st = x;
    return (int32_t)(x & ((1ull << bits) - 1));
}
__device__ __forceinline__ double xs_next_double(uint64_t& st) {
    const int64_t a = xs_next(st, 26);
    const int64_t b = xs_next(st, 27);
    return (double)((a << 27) + b) * 0x1.0p-53;
}
// GapSamplingIterator's skip for one draw
__device__ __forceinline__ int64_t gap_skip(uint64_t& st, double lnq) {
    double u = xs_next_double(st);
    if (u < 5e-11) u = 5e-11;
    const double q = log(u) / lnq;
    return q >= 2147483647.0 ? 2147483647 : (int64_t)q;
}

// Exclusive scan of v over the workgroup; *total gets the sum. sh holds kSampThreads entries.
__device__ __forceinline__ int64_t block_excl_scan(int64_t v, int64_t* sh, int64_t* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < kSampThreads; off <<= 1) {
        const int64_t t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const int64_t incl = sh[tid];
    *total = sh[kSampThreads - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kSampThreads) void sample_kernel(const ChainDesc* __restrict__ base,
                                                              ChainDesc* __restrict__ out,
                                                              const uint64_t* __restrict__ xs_state,
                                                              double fraction, int32_t* __restrict__ rows,
                                                              double* __restrict__ ys, int64_t stride) {
    __shared__ int64_t sh[kSampThreads];
    __shared__ int sh_emit;
    const int c = blockIdx.x;
    const int tid = threadIdx.x;
    ChainDesc dsc = base[c];
    int32_t* r = rows + (int64_t)c * stride;
    double* yo = ys ? ys + (int64_t)c * stride : nullptr;
    const double* Y = dsc.y;
    const int64_t nr = dsc.n_rows;
    uint64_t st = xs_state[c];
#pragma unroll 1
    for (int k = 0; k < 8; ++k)
        if ((tid >> k) & 1) st = gf2_apply(kSampleJumps.j[k], st);
    constexpr int64_t kRound = (int64_t)kSampThreads * kSampDraws;
    int64_t m = 0;
    if (fraction <= 0.4) {
        const double lnq = log1p(-fraction);
        int64_t pos_round = 0;   // the position before the round's first draw
        for (int64_t draw0 = 0;; draw0 += kRound) {
            uint64_t s = st;
            int64_t adv = 0;
            for (int j = 0; j < kSampDraws; ++j) adv += gap_skip(s, lnq) + 1;
            int64_t total;
            int64_t pos = pos_round + block_excl_scan(adv, sh, &total);
            if (tid == 0) sh_emit = 0;
            __syncthreads();
            s = st;
            int emitted = 0;
            const int64_t j0 = draw0 + (int64_t)tid * kSampDraws;
            for (int j = 0; j < kSampDraws; ++j) {
                pos += gap_skip(s, lnq);
                if (pos >= nr) break;
                r[j0 + j] = (int32_t)pos;
                if (yo) yo[j0 + j] = Y[pos];
                ++emitted;
                pos += 1;
            }
            atomicAdd(&sh_emit, emitted);
            __syncthreads();
            const int64_t e = sh_emit;
            pos_round += total;
            if (e < kRound) {   // a draw reached n_rows: the emitted draws are a prefix
                m = draw0 + e;
                break;
            }
            st = gf2_apply(kSampleJumps.j[8], st);
            __syncthreads();   // sh_emit is reset next round
        }
    } else {
        for (int64_t draw0 = 0; draw0 < nr; draw0 += kRound) {
            uint64_t s = st;
            uint64_t keep = 0;
            const int64_t t0 = draw0 + (int64_t)tid * kSampDraws;
            for (int j = 0; j < kSampDraws; ++j)
                if (xs_next_double(s) <= fraction && t0 + j < nr) keep |= 1ull << j;
            int64_t total;
            int64_t o = m + block_excl_scan(__popcll(keep), sh, &total);
            while (keep) {
                const int j = __ffsll((unsigned long long)keep) - 1;
                keep &= keep - 1;
                r[o] = (int32_t)(t0 + j);
                if (yo) yo[o] = Y[t0 + j];
                ++o;
            }
            m += total;
            st = gf2_apply(kSampleJumps.j[8], st);
        }
    }
    if (tid == 0) {
        dsc.rows = r;
        if (yo) dsc.y = yo;
        dsc.n_rows = m;
        out[c] = dsc;
    }
}

int launch_sample(const ChainDesc* base, ChainDesc* out, const uint64_t* xs_state, double fraction,
                  int32_t* rows, double* ys, int64_t stride, int n_chains, hipStream_t stream) {
    if (n_chains <= 0) return 0;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)n_chains), dim3(kSampThreads), 0, stream, base, out,
                       xs_state, fraction, rows, ys, stride);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// BernoulliCellSampler over the registered partitions (randomSplit, kFold): one
// nextDouble per row in iterator order, no gap sampling, so the filter branch of sample_kernel
// with a cell test in place of `<= fraction`. The partition's sampler seed is derived here from
// its global partition index (the host computes nothing): seed + index, or the index-th nextLong
// of java.util.Random(seed) reached by composing the LCG's step with itself (x -> A x + C mod
// 2^48, 2 steps a nextLong), then hashSeed (MurmurHash3 of the Long's 8 big-endian bytes and 56
// zeros, as sampling::xorshift_hash_seed in psgd_capi.cpp). Integer arithmetic and comparisons
// only; every output is placed by an exclusive scan, no atomics.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t cell_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

__device__ uint64_t cell_hash_seed(int64_t s) {
    uint32_t h = 0x3c074a61u;   // MurmurHash3.arraySeed
#pragma unroll 1
    for (int i = 0; i < 16; ++i) {
        // little-endian words of the big-endian Long followed by 56 zero bytes
        uint32_t k = i < 2 ? __builtin_bswap32((uint32_t)((uint64_t)s >> (32 - 32 * i))) : 0u;
        k *= 0xcc9e2d51u;
        k = cell_rotl32(k, 15);
        k *= 0x1b873593u;
        h ^= k;
        h = cell_rotl32(h, 13);
        h = h * 5u + 0xe6546b64u;
    }
    h ^= 64u;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return (uint64_t)(int64_t)(int32_t)h;
}

// The p-th (0-based) nextLong of java.util.Random(seed).
__device__ int64_t cell_java_long(int64_t seed, int64_t p) {
    constexpr uint64_t M = (1ull << 48) - 1;
    uint64_t x = ((uint64_t)seed ^ 0x5DEECE66Dull) & M;
    uint64_t a = 0x5DEECE66Dull, c = 0xBull, acc_a = 1, acc_c = 0;
#pragma unroll 1
    for (uint64_t n = 2 * (uint64_t)p; n; n >>= 1) {
        if (n & 1) {
            acc_a = (acc_a * a) & M;
            acc_c = (acc_c * a + c) & M;
        }
        c = ((a + 1) * c) & M;
        a = (a * a) & M;
    }
    x = (acc_a * x + acc_c) & M;
    x = (x * 0x5DEECE66Dull + 0xBull) & M;
    const int64_t hi = (int32_t)(uint32_t)(x >> 16);
    x = (x * 0x5DEECE66Dull + 0xBull) & M;
    const int64_t lo = (int32_t)(uint32_t)(x >> 16);
    return (int64_t)(((uint64_t)hi << 32) + (uint64_t)lo);
}

__global__ __launch_bounds__(kSampThreads) void cell_select_kernel(const ChainDesc* __restrict__ base,
                                                                   const int64_t* __restrict__ part_index,
                                                                   const int64_t* __restrict__ row_off, int csr,
                                                                   int64_t seed, int seeding, double lb, double ub,
                                                                   int complement, int32_t* __restrict__ rows,
                                                                   int64_t* __restrict__ counts,
                                                                   int64_t* __restrict__ nnz) {
    __shared__ int64_t sh[kSampThreads];
    const int c = blockIdx.x;
    const int tid = threadIdx.x;
    const ChainDesc dsc = base[c];
    const int64_t nr = dsc.n_rows;
    const int64_t p = part_index[c];
    const int64_t sp = seeding == 0 ? (int64_t)((uint64_t)seed + (uint64_t)p) : cell_java_long(seed, p);
    uint64_t st = cell_hash_seed(sp);
#pragma unroll 1
    for (int k = 0; k < 8; ++k)
        if ((tid >> k) & 1) st = gf2_apply(kSampleJumps.j[k], st);
    constexpr int64_t kRound = (int64_t)kSampThreads * kSampDraws;
    int32_t* r = rows + row_off[c];
    const int64_t* rp = csr ? dsc.row_ptr : nullptr;
    const bool comp = complement != 0;
    int64_t m = 0, len = 0;
    for (int64_t draw0 = 0; draw0 < nr; draw0 += kRound) {
        uint64_t s = st;
        uint64_t keep = 0;
        const int64_t t0 = draw0 + (int64_t)tid * kSampDraws;
        for (int j = 0; j < kSampDraws; ++j) {
            const double x = xs_next_double(s);
            const bool in = x >= lb && x < ub;
            if (in != comp && t0 + j < nr) keep |= 1ull << j;
        }
        int64_t total;
        int64_t o = m + block_excl_scan(__popcll(keep), sh, &total);
        while (keep) {
            const int j = __ffsll((unsigned long long)keep) - 1;
            keep &= keep - 1;
            r[o] = (int32_t)(t0 + j);
            if (rp) len += rp[t0 + j + 1] - rp[t0 + j];
            ++o;
        }
        m += total;
        st = gf2_apply(kSampleJumps.j[8], st);
    }
    int64_t total_len;
    block_excl_scan(len, sh, &total_len);
    if (tid == 0) {
        counts[c] = m;
        if (nnz) nnz[c] = total_len;
    }
}

int launch_cell_select(const ChainDesc* descs, const int64_t* part_index, const int64_t* row_off, int n_parts,
                       int layout, int64_t seed, int seeding, double lb, double ub, int complement, int32_t* rows,
                       int64_t* counts, int64_t* nnz, hipStream_t st) {
    if (n_parts <= 0) return 0;
    hipLaunchKernelGGL(cell_select_kernel, dim3((unsigned)n_parts), dim3(kSampThreads), 0, st, descs, part_index,
                       row_off, layout == kCsr ? 1 : 0, seed, seeding, lb, ub, complement, rows, counts, nnz);
    return (int)hipGetLastError();
}

int launch_steps(double step, int64_t n, double* steps, hipStream_t stream) {
    if (n <= 0) return 0;
    const int threads = 256;
    const int64_t blocks = (n + threads - 1) / threads;
    hipLaunchKernelGGL(steps_kernel, dim3((unsigned)blocks), dim3(threads), 0, stream, step, n, steps);
    return (int)hipGetLastError();
}

}  // namespace psgd
