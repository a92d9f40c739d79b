// The summary of one metric column over the replicates of a resampling study, shared by bootstrap.hip and calibration.hip:
// n_valid, mean and deviation (ddof = 1) summed in replicate order by one thread, then a bitonic sort of order-preserving 64-bit
// keys in LDS, NaN last, and numpy's linear percentile.  A workgroup of NT_COL threads owns one column.
#pragma once
#include "common.h"

#pragma clang fp contract(off)                                     // the sums below must not be fused: both users pin them to numpy

namespace {

constexpr int NT_COL = 256;                              // threads of a summary workgroup

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

// an order-preserving key of a double; every NaN is the largest key
__device__ __forceinline__ uint64_t sort_key(double v) {
  if (v != v) return ~0ull;
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// numpy's percentile, method "linear": position q (n - 1) between its neighbours, numpy's lerp
__device__ double percentile_sorted(const uint64_t* keys, int n, double q) {
  const double at = q * (double)(n - 1);
  double fl = floor(at);
  if (fl < 0.0) fl = 0.0;
  int i = (int)fl;
  if (i > n - 1) i = n - 1;
  const int j = i + 1 > n - 1 ? n - 1 : i + 1;
  const double t = at - (double)i, a = key_value(keys[i]), b = key_value(keys[j]), d = b - a;
  double r = t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
  if (t == 0.0) r = a;                                             // an infinite neighbour must not turn the bound into NaN
  if (t == 1.0) r = b;
  return r;
}

// s_val[0 .. B) holds the column in replicate order (all threads arrive after a barrier); s_key has n = a power of two >= B cells.
// summary[5][M]: n_valid, mean, std, low, high of column m.
__device__ void summarize_column(const double* s_val, uint64_t* s_key, int B, int n, int m, int M, double q_lo, double q_hi,
                                 double* __restrict__ summary) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += NT_COL) s_key[i] = i < B ? sort_key(s_val[i]) : ~0ull;
  int valid = 0;
  double mean = nan64(), dev = nan64();
  if (tid == 0) {                                                  // in replicate order, one owner
    double sum = 0.0;
    for (int i = 0; i < B; ++i) {
      const double v = s_val[i];
      if (v == v) { sum += v; ++valid; }
    }
    if (valid > 0) {
      mean = sum / (double)valid;
      double sq = 0.0;
      for (int i = 0; i < B; ++i) {
        const double v = s_val[i];
        if (v == v) sq += (v - mean) * (v - mean);
      }
      if (valid > 1) dev = sqrt(sq / (double)(valid - 1));
    }
  }
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < n; i += NT_COL) {
        const int o = i ^ j;                                       // o < n: n is a power of two and j < n
        if (o > i) {
          const uint64_t a = s_key[i], b = s_key[o];
          if ((a > b) == ((i & k) == 0)) { s_key[i] = b; s_key[o] = a; }
        }
      }
    }
  __syncthreads();
  if (tid == 0) {
    summary[m] = (double)valid;
    summary[M + m] = mean;
    summary[2 * M + m] = dev;
    summary[3 * M + m] = valid > 0 ? percentile_sorted(s_key, valid, q_lo) : nan64();
    summary[4 * M + m] = valid > 0 ? percentile_sorted(s_key, valid, q_hi) : nan64();
  }
}

// Dynamic LDS of a column workgroup: the B values (fp64) and n >= B sort keys (n a power of two, >= 2): at B = 8192, 128 KiB.
inline int pow2_at_least(int B) {
  int n = 2;
  while (n < B) n <<= 1;
  return n;
}
inline size_t column_lds_bytes(int B) { return ((size_t)B + pow2_at_least(B)) * 8; }

}  // namespace
