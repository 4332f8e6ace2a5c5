// psgd_mathprobe.hip -- the per-sample scalar functions of psgd_device.h, applied elementwise to
// device arrays (gfx950). The chain kernels evaluate these once per row from a dot product, so
// their suite only ever feeds them the margins its data produces; this entry feeds them any
// argument (tests/test_gpu_math_edges.py: every binade, the clamp and overflow edges, the
// rint half-way points, non-finite values). It calls the functions the kernels call, compiled
// with the kernels' flags; it is not part of the C ABI (reached by its mangled name).
#include "psgd_device.h"

namespace psgd {

// op codes; + G_LOGISTIC / G_LEAST_SQUARES / G_HINGE where the function is a template on GRAD.
// f64 ops read a, b and write out0, out1 as double, f32 ops as float. b is the second argument
// where there is one (iter; the label y; pow's exponent), out1 the loss where there is one.
enum {
    MP_RECIP_ONE_PLUS_EXP = 0,   // recip_one_plus_exp(a)
    MP_RECIP_NEWTON = 1,
    MP_RSQRT_NEWTON = 2,
    MP_SQRT_NEWTON = 3,
    MP_ONE_MINUS_POW_ITER = 4,   // one_minus_pow_iter(a, b)
    MP_LOG1P_EXP64 = 5,          // log1p_exp<double>(a)
    MP_ONE_MINUS_POW64 = 6,      // 1.0 - m_pow(a, b): what one_minus_pow_iter must equal bit for bit
    MP_COEF64 = 10,              // coef64<G>(z = a, y = b, ns = 1): mult
    MP_GRADIENT64 = 20,          // gradient_scalar<G, double>(z = a, y = b): mult, loss
    MP_COEF32 = 30,              // coef<G>(a, y = b, s = 1, ns = -1, aux): -mult (Logistic: a = u)
    MP_ROW_LOSS32 = 40,          // row_loss<G>(z = a, y = b, aux)
    MP_SPARSE_COEF = 50,         // sparse_coef<G>(z = a, y = b, s = 1): -mult, loss
    MP_SPLIT_SIGMOID = 60,       // sigmoid_mult_fast(z = a, y = b)
    MP_GRADIENT32 = 70,          // gradient_scalar<G, float>(z = a, y = b): mult, loss
    MP_POW_FAST = 80,            // pow_fast(a, b)
};

namespace {

// chain_block's aux operand: s*y (s = 1) for LeastSquares and Logistic, ls = 2y - 1 for Hinge
template <int GRAD>
__device__ __forceinline__ float aux_of(float y) {
    return GRAD == G_HINGE ? 2.0f * y - 1.0f : y;
}

template <int OP, int GRAD>
__global__ __launch_bounds__(256) void math_probe64_kernel(int64_t n, const double* __restrict__ a,
                                                           const double* __restrict__ b,
                                                           double* __restrict__ o0, double* __restrict__ o1) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b[i];
    double r0 = 0.0, r1 = 0.0;
    if constexpr (OP == MP_RECIP_ONE_PLUS_EXP) r0 = recip_one_plus_exp(x);
    else if constexpr (OP == MP_RECIP_NEWTON) r0 = recip_newton(x);
    else if constexpr (OP == MP_RSQRT_NEWTON) r0 = rsqrt_newton(x);
    else if constexpr (OP == MP_SQRT_NEWTON) r0 = sqrt_newton(x);
    else if constexpr (OP == MP_ONE_MINUS_POW_ITER) r0 = one_minus_pow_iter(x, y);
    else if constexpr (OP == MP_LOG1P_EXP64) r0 = log1p_exp<double>(x);
    else if constexpr (OP == MP_ONE_MINUS_POW64) r0 = 1.0 - m_pow(x, y);
    else if constexpr (OP == MP_COEF64) r0 = coef64<GRAD>(x, y, 1.0);
    else r1 = gradient_scalar<GRAD, double>(x, y, r0);
    o0[i] = r0;
    o1[i] = r1;
}

template <int OP, int GRAD>
__global__ __launch_bounds__(256) void math_probe32_kernel(int64_t n, const float* __restrict__ a,
                                                           const float* __restrict__ b,
                                                           float* __restrict__ o0, float* __restrict__ o1) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = a[i], y = b[i];
    float r0 = 0.0f, r1 = 0.0f;
    if constexpr (OP == MP_COEF32) r0 = coef<GRAD>(x, y, 1.0f, -1.0f, aux_of<GRAD>(y));
    else if constexpr (OP == MP_ROW_LOSS32) r0 = row_loss<GRAD>(x, y, aux_of<GRAD>(y));
    else if constexpr (OP == MP_SPARSE_COEF) r0 = sparse_coef<GRAD>(x, y, 1.0f, r1);
    else if constexpr (OP == MP_SPLIT_SIGMOID) r0 = sigmoid_mult_fast(x, y);
    else if constexpr (OP == MP_GRADIENT32) r1 = gradient_scalar<GRAD, float>(x, y, r0);
    else r0 = pow_fast(x, y);
    o0[i] = r0;
    o1[i] = r1;
}

template <int OP, int GRAD>
void launch64(int64_t n, const void* a, const void* b, void* o0, void* o1, hipStream_t st) {
    hipLaunchKernelGGL((math_probe64_kernel<OP, GRAD>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n,
                       (const double*)a, (const double*)b, (double*)o0, (double*)o1);
}
template <int OP, int GRAD>
void launch32(int64_t n, const void* a, const void* b, void* o0, void* o1, hipStream_t st) {
    hipLaunchKernelGGL((math_probe32_kernel<OP, GRAD>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n,
                       (const float*)a, (const float*)b, (float*)o0, (float*)o1);
}
template <int OP>
bool launch64_grad(int g, int64_t n, const void* a, const void* b, void* o0, void* o1, hipStream_t st) {
    switch (g) {
    case G_LOGISTIC: launch64<OP, G_LOGISTIC>(n, a, b, o0, o1, st); return true;
    case G_LEAST_SQUARES: launch64<OP, G_LEAST_SQUARES>(n, a, b, o0, o1, st); return true;
    case G_HINGE: launch64<OP, G_HINGE>(n, a, b, o0, o1, st); return true;
    default: return false;
    }
}
template <int OP>
bool launch32_grad(int g, int64_t n, const void* a, const void* b, void* o0, void* o1, hipStream_t st) {
    switch (g) {
    case G_LOGISTIC: launch32<OP, G_LOGISTIC>(n, a, b, o0, o1, st); return true;
    case G_LEAST_SQUARES: launch32<OP, G_LEAST_SQUARES>(n, a, b, o0, o1, st); return true;
    case G_HINGE: launch32<OP, G_HINGE>(n, a, b, o0, o1, st); return true;
    default: return false;
    }
}

}  // namespace

// Applies function `op` to a[i] (and b[i]) for i < n; all four arrays are device arrays of n
// doubles (op < MP_COEF32) or floats. Returns 0, -1 for an unknown op or a null array, or the
// HIP error of the launch.
int math_probe(int op, int64_t n, const void* a, const void* b, void* out0, void* out1, hipStream_t st) {
    if (n < 0 || n > ((int64_t)1 << 30) || !a || !b || !out0 || !out1) return -1;
    if (n == 0) return 0;
    bool ok = true;
    switch (op) {
    case MP_RECIP_ONE_PLUS_EXP: launch64<MP_RECIP_ONE_PLUS_EXP, 0>(n, a, b, out0, out1, st); break;
    case MP_RECIP_NEWTON: launch64<MP_RECIP_NEWTON, 0>(n, a, b, out0, out1, st); break;
    case MP_RSQRT_NEWTON: launch64<MP_RSQRT_NEWTON, 0>(n, a, b, out0, out1, st); break;
    case MP_SQRT_NEWTON: launch64<MP_SQRT_NEWTON, 0>(n, a, b, out0, out1, st); break;
    case MP_ONE_MINUS_POW_ITER: launch64<MP_ONE_MINUS_POW_ITER, 0>(n, a, b, out0, out1, st); break;
    case MP_LOG1P_EXP64: launch64<MP_LOG1P_EXP64, 0>(n, a, b, out0, out1, st); break;
    case MP_ONE_MINUS_POW64: launch64<MP_ONE_MINUS_POW64, 0>(n, a, b, out0, out1, st); break;
    case MP_SPLIT_SIGMOID: launch32<MP_SPLIT_SIGMOID, 0>(n, a, b, out0, out1, st); break;
    case MP_POW_FAST: launch32<MP_POW_FAST, 0>(n, a, b, out0, out1, st); break;
    default:
        if (op >= MP_COEF64 && op < MP_COEF64 + 3) ok = launch64_grad<MP_COEF64>(op - MP_COEF64, n, a, b, out0, out1, st);
        else if (op >= MP_GRADIENT64 && op < MP_GRADIENT64 + 3) ok = launch64_grad<MP_GRADIENT64>(op - MP_GRADIENT64, n, a, b, out0, out1, st);
        else if (op >= MP_COEF32 && op < MP_COEF32 + 3) ok = launch32_grad<MP_COEF32>(op - MP_COEF32, n, a, b, out0, out1, st);
        else if (op >= MP_ROW_LOSS32 && op < MP_ROW_LOSS32 + 3) ok = launch32_grad<MP_ROW_LOSS32>(op - MP_ROW_LOSS32, n, a, b, out0, out1, st);
        else if (op >= MP_SPARSE_COEF && op < MP_SPARSE_COEF + 3) ok = launch32_grad<MP_SPARSE_COEF>(op - MP_SPARSE_COEF, n, a, b, out0, out1, st);
        else if (op >= MP_GRADIENT32 && op < MP_GRADIENT32 + 3) ok = launch32_grad<MP_GRADIENT32>(op - MP_GRADIENT32, n, a, b, out0, out1, st);
        else ok = false;
    }
    if (!ok) return -1;
    return (int)hipGetLastError();
}

}  // namespace psgd
