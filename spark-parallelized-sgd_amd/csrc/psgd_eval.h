// psgd_eval.h -- device helpers the passes at fixed weights share (psgd_eval.hip, psgd_eval_mn.hip,
// psgd_grad.hip, psgd_grad_mn.hip).
#pragma once
#include "psgd_device.h"

namespace psgd {

// The multinomial passes' row hold and margin buffer (psgd_eval_mn.hip's header tells the layout).
constexpr int kMnHold = 8;             // dense: elements of a row a lane holds
constexpr int kMnRows = 2;             // dense: rows a lane group holds (a weight read serves both)
constexpr int kMnCsrHold = 4;          // CSR: entries of a row a lane holds
constexpr int kMnBuf = 384;            // doubles of a wave's margin buffer, row-per-lane softmax
constexpr int kMnLdsMax = 144 * 1024;  // a workgroup's LDS at most (the wide softmax's buffers)

// Sum over aligned groups of gl (a power of two, wave-uniform) lanes: the first log2(gl) steps of
// wave_sum. Every lane of a group ends with the same bits.
__device__ __forceinline__ double group_sum(double v, int gl) {
    if (gl > 1) v = v + dpp_mov<0xB1>(v);    // quad_perm [1,0,3,2]
    if (gl > 2) v = v + dpp_mov<0x4E>(v);    // quad_perm [2,3,0,1]
    if (gl > 4) v = v + dpp_mov<0x141>(v);   // row_half_mirror
    if (gl > 8) v = v + dpp_mov<0x140>(v);   // row_mirror
    if (gl > 16) v = swap_sum16(v);
    if (gl > 32) v = swap_sum32(v);
    return v;
}

// group_sum of two values at once: the same operations on each, the two dependent chains interleaved.
__device__ __forceinline__ void group_sum2(double& a, double& b, int gl) {
    if (gl > 1) { const double pa = dpp_mov<0xB1>(a), pb = dpp_mov<0xB1>(b); a = a + pa; b = b + pb; }
    if (gl > 2) { const double pa = dpp_mov<0x4E>(a), pb = dpp_mov<0x4E>(b); a = a + pa; b = b + pb; }
    if (gl > 4) { const double pa = dpp_mov<0x141>(a), pb = dpp_mov<0x141>(b); a = a + pa; b = b + pb; }
    if (gl > 8) { const double pa = dpp_mov<0x140>(a), pb = dpp_mov<0x140>(b); a = a + pa; b = b + pb; }
    if (gl > 16) { const double sa = swap_sum16(a), sb = swap_sum16(b); a = sa; b = sb; }
    if (gl > 32) { const double sa = swap_sum32(a), sb = swap_sum32(b); a = sa; b = sb; }
}

// The item's partition: the last p with first tile <= item (empty partitions share their first
// tile with the next one, so the last such p is the one that owns the tile). Wave-uniform.
__device__ __forceinline__ int item_partition(const EvalPart* ep, int P, int64_t item) {
    const int64_t base = ep[0].tile0;
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ep[mid].tile0 - base <= item) lo = mid; else hi = mid;
    }
    return lo;
}

// The tile's partition: the last p with tile0[p] <= tile. Wave-uniform.
__device__ __forceinline__ int tile_partition(const int64_t* tile0, int P, int64_t tile) {
    int lo = 0, hi = P;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile0[mid] <= tile) lo = mid; else hi = mid;
    }
    return lo;
}

// Double.toInt
__device__ __forceinline__ int mn_d2i(double x) {
    if (x != x) return 0;
    if (x >= 2147483647.0) return 2147483647;
    if (x <= -2147483648.0) return (-2147483647 - 1);
    return (int)x;
}

// The loss from the pieces (Gradient.scala, numClasses > 2): sum is the sum of exponentials of the
// (shifted) margins, M the maximum margin.
__device__ __forceinline__ double mn_loss(double sum, double marginY, double M, double y) {
    double loss = y > 0.0 ? log1p(sum) - marginY : log1p(sum);
    if (M > 0.0) loss = loss + M;
    return loss;
}

// The margin buffer's shape for a partition whose wave pass could take `rpw` groups of `rows` rows:
// pitch of a row, groups a pass uses (rp <= rpw) and rows the buffer holds before it is scored (nb, a
// multiple of rp * rows).
template <bool ROWLANE>
__device__ __forceinline__ void mn_buffer_shape(int C1, int rpw, int rows, int& pitch, int& rp, int& nb) {
    if constexpr (ROWLANE) {
        pitch = C1 | 1;   // odd: the lanes' rows start on different banks
        int cap = kMnBuf / pitch;
        cap = cap > 64 ? 64 : cap;
        rp = cap / rows < rpw ? cap / rows : rpw;
        nb = (cap / (rp * rows)) * (rp * rows);
    } else {
        pitch = C1;
        rp = 1;
        nb = rows;
    }
}

// A wave's own LDS buffer changes hands between its lanes: order the accesses within the wave.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
}  // namespace psgd
