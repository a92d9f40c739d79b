// Device functions the forward-only image explainers share after their model forwards (rise.hip's accumulate,
// faithfulness.hip's curves): the class an image is explained on and the fp64 soft-max probability of a class.
// tests/rise_oracle.py and tests/faithfulness_oracle.py restate both in this operation order.
//
// Not here, on purpose: the two fixed-order fp64 workgroup sums.  block_tree_sum (faithfulness.hip) halves an LDS array of
// one partial per thread; block_sum_f64 (uncertainty.hip) sums each wave by shuffles and then adds the wave totals in ascending
// order.  The orders differ, the results differ in the last bits, and each has tests that pin its own.
#pragma once
#include "common.h"

constexpr int TARGET_MAX_CLASSES = 65536;   // K of the entry points that call these: a thread walks a row of logits serially

// The class image n is explained on, from its clean logits l[0 .. K): the given target clamped to what exists, else the first
// largest logit, where a NaN is never larger (an all-NaN row gives class 0).
__device__ __forceinline__ int pick_target(const float* __restrict__ l, int K, const int32_t* __restrict__ target_in, int n) {
  int t;
  if (target_in) {
    t = min(max(target_in[n], 0), K - 1);
  } else {
    t = 0;
    float best = l[0];
    for (int c = 1; c < K; ++c) {
      const float v = l[c];
      if (v > best || (best != best && v == v)) { best = v; t = c; }
    }
  }
  return t;
}

// fp64 soft-max probability of class t of one row of K logits: the maximum, then the sum of exp(l - max) in ascending class order
__device__ __forceinline__ double row_probability(const float* __restrict__ l, int K, int t) {
  double mx = (double)l[0];
  for (int c = 1; c < K; ++c) mx = fmax(mx, (double)l[c]);
  double sum = 0.0;
  for (int c = 0; c < K; ++c) sum = sum + exp((double)l[c] - mx);
  return exp((double)l[t] - mx) / sum;
}
