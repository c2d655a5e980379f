// kernels_rows.hpp -- what the "one wave per row" evaluation kernels share (kernels_trace / _energy / _metrics / _joint / _ais /
// _reverse_ais / _bound / _knn .hpp).
//
//   rows      a block is ROW_WAVES waves and wave w of block b takes row ROW_WAVES b + w (wave_row); lane l of that wave (wave_lane)
//             takes the row's elements l, l + 64, ... in ascending order.
//   sums      the 64 lane values meet in the xor butterfly 32, 16, .. 1 and every lane ends with the result (wave_sum_all,
//             wave_max_all), so a row's sum has one order whatever the batch around it.  kernels_ew.hpp's wave_sum is the other
//             reduction -- __shfl_down, result in lane 0 only -- and serves the propagation epilogues.
//   labels    a row of K <= LABEL_KMAX label values sits in registers: label c in lane c & 63, slot c >> 6 (slots_*); slots past K
//             hold 0.  Maxima follow torch.argmax / topk: the larger value first, the lower index on ties, NaN never wins.
#pragma once
#include "common.hpp"

namespace imdbn {

constexpr int ROW_WAVES = 4;                     // rows (waves) per block
constexpr int LABEL_KMAX = 256;                  // label window <= GROUP_WMAX: 4 slots of 64 lanes

__device__ __forceinline__ int wave_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ int wave_row() { return blockIdx.x * ROW_WAVES + (threadIdx.x >> 6); }

template <class T>                               // float, double, int
__device__ __forceinline__ T wave_sum_all(T v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <class T>                               // float, double
__device__ __forceinline__ T wave_max_all(T v) {
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// (value, index) ordering of torch.argmax / topk: larger value first, the lower index on ties
__device__ __forceinline__ bool vi_better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// a row of K floats into the slots
__device__ __forceinline__ void slots_load(float (&v)[4], const float* row, int l, int K) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = l + 64 * q;
        v[q] = c < K ? row[c] : 0.f;
    }
}

// index of the first maximum, the same in every lane; `none` for a row in which nothing wins (all NaN)
__device__ __forceinline__ int slots_argmax(const float (&v)[4], int l, int K, int none = 0x7fffffff) {
    float best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = l + 64 * q;
        if (c < K && vi_better(v[q], c, best, bi)) { best = v[q]; bi = c; }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const float w = __shfl_xor(best, o); const int j = __shfl_xor(bi, o);
        if (vi_better(w, j, best, bi)) { best = w; bi = j; }
    }
    return bi < K ? bi : none;
}

// the two largest values and their indices, the same in every lane: per lane over its slots, then a butterfly that merges two sorted
// top-2 lists
struct Top2 { float v1, v2; int i1, i2; };
__device__ __forceinline__ Top2 slots_top2(const float (&y)[4], int l, int K) {
    float v1 = -INFINITY, v2 = -INFINITY; int i1 = 0x7fffffff, i2 = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = l + 64 * q;
        const float yq = y[q];
        if (c < K) {
            if (vi_better(yq, c, v1, i1)) { v2 = v1; i2 = i1; v1 = yq; i1 = c; }
            else if (vi_better(yq, c, v2, i2)) { v2 = yq; i2 = c; }
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const float w1 = __shfl_xor(v1, o), w2 = __shfl_xor(v2, o);
        const int j1 = __shfl_xor(i1, o), j2 = __shfl_xor(i2, o);
        if (vi_better(v1, i1, w1, j1)) {
            if (vi_better(w1, j1, v2, i2)) { v2 = w1; i2 = j1; }
        } else {
            if (vi_better(v1, i1, w2, j2)) { v2 = v1; i2 = i1; } else { v2 = w2; i2 = j2; }
            v1 = w1; i1 = j1;
        }
    }
    return Top2{v1, v2, i1, i2};
}

// the value of label k (wave-uniform) in every lane; 0 for a k outside [0, LABEL_KMAX)
template <class T>                               // float, double
__device__ __forceinline__ T slots_pick(const T (&v)[4], int k) {
    const int q = k >> 6;
    const T sel = q == 0 ? v[0] : q == 1 ? v[1] : q == 2 ? v[2] : q == 3 ? v[3] : (T)0;
    return __shfl(sel, k & 63);
}

}  // namespace imdbn
