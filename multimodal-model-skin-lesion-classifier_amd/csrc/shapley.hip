// Shapley values of the metadata COLUMNS on the model itself (mmskin.shapley.MetadataShapley): the two kernels on either side of
// the batched fusion-head calls.  The reference explains a random-forest surrogate of the recorded probabilities, one one-hot
// cell per feature (src/scripts/data_preprocessing/shap_values.py); here the players are the encoder's columns, the value
// function is the network, and the image is encoded once.
//
// The estimator.  M = n_cat + n_num players, G background rows b_g, P permutations pi_p of 0 .. M-1, an explained row x:
//     v(S) = (1/G) sum_g out(fuse(f, mix(x, b_g, S)))          mix: column j from x if j in S, else from b_g
//     phi_j = (1/2P) sum_p [ v(S_{q+1}) - v(S_q) + v(T_{M-q}) - v(T_{M-q-1}) ]      q = position of j in pi_p,
// S_n = the first n entries of pi_p, T_n = its last n entries (the antithetic walk: the same permutation from both ends).
// S_0 = T_0 = the empty coalition, S_M = T_M = all columns: both are evaluated once per sample, not once per permutation.
//
// The row order (include/mmskin.h states it for callers).  With K = 2 P (M - 1) interior coalitions per sample:
//     rows [0, B (K+1) G)              row = ((b (K+1) + k) G + g):   sample b, coalition k, background row g;
//                                      k = (p 2 + side) (M-1) + (n-1) is S_n (side 0) or T_n (side 1) of pi_p, n = 1 .. M-1,
//                                      and k = K is the empty coalition (the G rows of v(empty))
//     rows [B (K+1) G, B (K+1) G + B)  row b of this block is x_b itself (v(all), one row)
// so every coalition starts on a multiple of G and a row range cut at multiples of G never splits one.
//
//   coalitions  raw codes / numerics of x and of the background + the inverse permutation table -> the encoded metadata rows of
//               a row range.  One thread per output element, every element written exactly once, no atomics; the cell is
//               meta_encode.h's, the one metadata_encode_kernel (preprocess.hip) and metadata_variants_kernel (sweep.hip) call,
//               so a row equals the encoding of the mixed raw row bit for bit.
//   value       logits of a row range -> v: soft-max (or nothing), then the mean over the G rows of each coalition in fp64.  One
//               wave serves one coalition; it holds 64 / cpad rows at a time (cpad = C rounded up to a power of two, one lane
//               per class), each row group sums its rows g, g + 64 / cpad, ... in that order, and the groups are then added in a
//               fixed xor tree.  No atomics: v does not depend on the launch order.
//   phi         one thread per (b, j, c): the four-term marginals of column j, summed over p = 0 .. P-1 in fp64.
//   accumulate  one thread per (j, c): |phi| added over b = 0 .. B-1, in that order, into the caller's fp64 [M][C] sums.
//
// tests/shapley_oracle.py restates all of it in numpy.
#include "../../include/mmskin.h"
#include "common.h"
#include "meta_encode.h"

#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                  // threads per workgroup
constexpr int MAX_C = 64;                // value: one lane per class

// ------------------------------------------------------------------------------------------------ coalitions
__global__ __launch_bounds__(NT) void shapley_coalitions_kernel(const int32_t* __restrict__ codes, const float* __restrict__ numeric,
                                                                const int32_t* __restrict__ bg_codes, const float* __restrict__ bg_numeric,
                                                                int n_cat, const int32_t* __restrict__ col_offset, int onehot_width,
                                                                int n_num, const float* __restrict__ mean, const float* __restrict__ scale,
                                                                float nan_fill, const int32_t* __restrict__ pos, int G, int P, int M,
                                                                int64_t row0, int64_t n_rows, int64_t coalition_rows, int out_width,
                                                                float* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x;
  if (i >= n_rows * out_width) return;
  const int j = (int)(i % out_width);
  const int64_t r = row0 + i / out_width;
  float v = 0.f;                                                 // columns past the encoder's width
  if (j < onehot_width + n_num) {
    const int col = j < onehot_width ? meta_slot_column(j, n_cat, col_offset) : n_cat + (j - onehot_width);
    // does the explained row supply this column (col in the coalition), or background row g?
    int b, g = 0;
    bool own = true;
    if (r >= coalition_rows) {
      b = (int)(r - coalition_rows);                              // v(all)
    } else {
      const int walk = 2 * (M - 1), K = P * walk;
      const int64_t u = r / G;
      g = (int)(r - u * G);
      b = (int)(u / (K + 1));
      const int k = (int)(u - (int64_t)b * (K + 1));
      if (k == K) {
        own = false;                                              // v(empty)
      } else {
        const int p = k / walk, rem = k - p * walk;
        const int side = rem >= M - 1, n = rem - side * (M - 1) + 1;
        const int q = pos[p * M + col];
        own = side ? q >= M - n : q < n;
      }
    }
    if (j < onehot_width) {
      const int code = own ? codes[(int64_t)b * n_cat + col] : bg_codes[(int64_t)g * n_cat + col];
      v = meta_onehot_cell(code, j, col_offset[col]);
    } else {
      const int k = j - onehot_width;
      const float x = own ? numeric[(int64_t)b * n_num + k] : bg_numeric[(int64_t)g * n_num + k];
      v = meta_numeric_cell(x, mean[k], scale[k], nan_fill);
    }
  }
  out[i] = v;
}

// ------------------------------------------------------------------------------------------------ value
// reductions over the aligned groups of `width` lanes (a power of two): every lane of a group ends with its group's result
__device__ __forceinline__ float group_max(float v, int width) {
  for (int o = width >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float group_sum(float v, int width) {
  for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// units [unit0, unit0 + n_units): a unit below `coalitions` is coalition u (G rows from row u G), the others are the v(all) rows
template <typename T>
__global__ __launch_bounds__(NT) void shapley_value_kernel(const T* __restrict__ logits, int C, int cpad, int G, int K, int output,
                                                           int64_t row0, int64_t unit0, int64_t n_units, int64_t coalitions,
                                                           double* __restrict__ v) {
  const int lane = threadIdx.x & 63;
  const int64_t u = unit0 + blockIdx.x * (int64_t)(NT / 64) + (threadIdx.x >> 6);
  if (u >= unit0 + n_units) return;                             // uniform per wave: the shuffles below see all 64 lanes
  const int c = lane & (cpad - 1), group = lane / cpad, groups = 64 / cpad;
  const bool live = c < C;
  const bool whole = u >= coalitions;
  const int64_t first = whole ? coalitions * G + (u - coalitions) : u * G;
  const int rows = whole ? 1 : G;
  const T* src = logits + (first - row0) * C;
  double acc = 0.0;
  for (int g0 = 0; g0 < rows; g0 += groups) {
    const int g = g0 + group;
    const bool on = live && g < rows;
    const float x = on ? to_f32(src[(int64_t)g * C + c]) : -INFINITY;
    float val = x;
    if (output == MMSKIN_SHAPLEY_PROB) {                          // exp(x - max) / sum, as torch.softmax and sweep_reduce
      const float top = group_max(x, cpad);
      const float e = on ? expf(x - top) : 0.f;
      val = e / group_sum(e, cpad);
    }
    if (on) acc += (double)val;
  }
  for (int o = cpad; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);   // the row groups, in a fixed tree
  if (group == 0 && live) {
    const int64_t b = whole ? u - coalitions : u / (K + 1);
    const int64_t k = whole ? K + 1 : u - b * (K + 1);
    v[(b * (K + 2) + k) * C + c] = acc / (double)rows;
  }
}

// ------------------------------------------------------------------------------------------------ phi
__global__ __launch_bounds__(NT) void shapley_phi_kernel(const double* __restrict__ v, const int32_t* __restrict__ pos, int B, int P,
                                                         int M, int C, float* __restrict__ phi, float* __restrict__ base,
                                                         float* __restrict__ full) {
  const int64_t i = blockIdx.x * (int64_t)NT + threadIdx.x;
  if (i >= (int64_t)B * M * C) return;
  const int c = (int)(i % C), j = (int)((i / C) % M);
  const int64_t b = i / ((int64_t)C * M);
  const int K = 2 * P * (M - 1);
  const double* vb = v + b * (K + 2) * C + c;
  const double v_empty = vb[(int64_t)K * C], v_all = vb[(int64_t)(K + 1) * C];
  // v of the first (side 0) or last (side 1) n entries of permutation p
  auto at = [&](int p, int side, int n) {
    return n == 0 ? v_empty : n == M ? v_all : vb[(int64_t)((p * 2 + side) * (M - 1) + n - 1) * C];
  };
  double sum = 0.0;
  for (int p = 0; p < P; ++p) {
    const int q = pos[p * M + j];
    sum += (at(p, 0, q + 1) - at(p, 0, q)) + (at(p, 1, M - q) - at(p, 1, M - q - 1));
  }
  phi[i] = (float)(sum / (2.0 * P));
  if (j == 0) {
    base[b * C + c] = (float)v_empty;
    full[b * C + c] = (float)v_all;
  }
}

__global__ __launch_bounds__(NT) void shapley_accumulate_kernel(const float* __restrict__ phi, int B, int MC, double* __restrict__ abs_sum) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= MC) return;
  double a = abs_sum[i];
  for (int b = 0; b < B; ++b) a += fabs((double)phi[(int64_t)b * MC + i]);
  abs_sum[i] = a;
}

// ------------------------------------------------------------------------------------------------ host
// the walk's extents, checked once for both entry points; `what` names the caller in the message
int walk_extents(const char* what, int batch, int G, int P, int M, int64_t* coalition_rows, int64_t* rows) {
  ARG_CHECK(batch >= 1 && G >= 1 && P >= 1 && M >= 1, "%s: every extent must be >= 1 (batch %d, G %d, P %d, M %d)", what, batch, G, P, M);
  ARG_CHECK(M <= (1 << 12) && (int64_t)P * M <= (1 << 20), "%s: %d permutations of %d columns are out of range", what, P, M);
  const int64_t K = 2 * (int64_t)P * (M - 1);
  ARG_CHECK((K + 2) * batch < ((int64_t)1 << 31) / MAX_C && (K + 1) * batch * G < ((int64_t)1 << 40), "%s: %d x %d x %d x %d rows are out of "
            "range", what, batch, G, P, M);
  *coalition_rows = (K + 1) * batch * G;
  *rows = *coalition_rows + batch;
  return MMSKIN_OK;
}

// every row of the table is a permutation of 0 .. M-1 -> pos[p][perm[p][n]] = n, uploaded into pos_scratch on `stream`
int upload_positions(const char* what, const int32_t* perm_host, int P, int M, int32_t* pos_scratch, void* stream) {
  std::vector<int32_t> pos((size_t)P * M, -1);
  for (int p = 0; p < P; ++p)
    for (int n = 0; n < M; ++n) {
      const int32_t j = perm_host[(size_t)p * M + n];
      ARG_CHECK(j >= 0 && j < M && pos[(size_t)p * M + j] < 0, "%s: row %d of the table is not a permutation of 0 .. %d (entry %d is %d)", what,
                p, M - 1, n, j);
      pos[(size_t)p * M + j] = n;
    }
  // pageable host memory: the copy has left the host buffer when hipMemcpyAsync returns
  HIP_CHECK_RET(hipMemcpyAsync(pos_scratch, pos.data(), pos.size() * sizeof(int32_t), hipMemcpyHostToDevice, ST(stream)));
  return MMSKIN_OK;
}

}  // namespace

extern "C" int64_t mmskin_shapley_rows(int batch, int G, int P, int M) {
  int64_t coalition_rows = 0, rows = 0;
  return walk_extents("shapley_rows", batch, G, P, M, &coalition_rows, &rows) == MMSKIN_OK ? rows : -1;
}

extern "C" int mmskin_shapley_coalitions(const int32_t* codes, const float* numeric, int batch, const int32_t* bg_codes,
                                         const float* bg_numeric, int G, int n_cat, const int32_t* col_offset,
                                         const int32_t* col_offset_host, int onehot_width, int n_num, const float* mean, const float* scale,
                                         float nan_fill, const int32_t* perm_host, int32_t* pos_scratch, int P, int64_t row0, int64_t row1,
                                         float* out, int out_width, void* stream) {
  if (int rc = check_meta_layout("shapley_coalitions", n_cat, n_num, onehot_width, col_offset, col_offset_host)) return rc;
  const int M = n_cat + n_num;
  int64_t coalition_rows = 0, rows = 0;
  if (int rc = walk_extents("shapley_coalitions", batch, G, P, M, &coalition_rows, &rows)) return rc;
  ARG_CHECK(out_width >= 1 && out_width <= (1 << 20), "shapley_coalitions: out_width %d is out of range", out_width);
  ARG_CHECK(row0 >= 0 && row0 < row1 && row1 <= rows, "shapley_coalitions: rows [%lld, %lld) are not a range of the walk's %lld rows",
            (long long)row0, (long long)row1, (long long)rows);
  ARG_CHECK((row1 - row0) * out_width < ((int64_t)1 << 38), "shapley_coalitions: %lld rows x %d are out of range", (long long)(row1 - row0),
            out_width);
  ARG_CHECK(out && perm_host && pos_scratch && ((codes && bg_codes) || n_cat == 0) && (n_num == 0 || (numeric && bg_numeric && mean && scale)),
            "shapley_coalitions: null argument");
  if (int rc = upload_positions("shapley_coalitions", perm_host, P, M, pos_scratch, stream)) return rc;
  const int64_t total = (row1 - row0) * out_width;
  hipLaunchKernelGGL(shapley_coalitions_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ST(stream), codes, numeric, bg_codes,
                     bg_numeric, n_cat, col_offset, onehot_width, n_num, mean, scale, nan_fill, pos_scratch, G, P, M, row0, row1 - row0,
                     coalition_rows, out_width, out);
  HIP_CHECK_RET(hipGetLastError());
  return MMSKIN_OK;
}

extern "C" int mmskin_shapley_reduce(const void* logits, int logits_dtype, int output, int batch, int G, int P, int M, int C, int64_t row0,
                                     int64_t row1, double* v, int finish, const int32_t* perm_host, int32_t* pos_scratch, float* phi,
                                     float* base, float* full, double* abs_sum, void* stream) {
  int64_t coalition_rows = 0, rows = 0;
  if (int rc = walk_extents("shapley_reduce", batch, G, P, M, &coalition_rows, &rows)) return rc;
  if (C < 2 || C > MAX_C) {
    mmskin_set_error("shapley_reduce: %d classes; the kernel holds one class per lane, 2 .. %d", C, MAX_C);
    return MMSKIN_ERR_UNSUPPORTED;
  }
  ARG_CHECK(logits_dtype == 0 || logits_dtype == 1, "shapley_reduce: logits dtype %d is neither fp32 (0) nor bf16 (1)", logits_dtype);
  ARG_CHECK(output == MMSKIN_SHAPLEY_PROB || output == MMSKIN_SHAPLEY_LOGIT, "shapley_reduce: output %d is neither PROB (0) nor LOGIT (1)",
            output);
  ARG_CHECK(row0 >= 0 && row0 <= row1 && row1 <= rows, "shapley_reduce: rows [%lld, %lld) are not a range of the walk's %lld rows",
            (long long)row0, (long long)row1, (long long)rows);
  ARG_CHECK((row0 >= coalition_rows || row0 % G == 0) && (row1 >= coalition_rows || row1 % G == 0), "shapley_reduce: rows [%lld, %lld) split a "
            "coalition: cut the walk at multiples of G = %d", (long long)row0, (long long)row1, G);
  ARG_CHECK(v && (logits || row0 == row1), "shapley_reduce: null argument");
  ARG_CHECK(!finish || (perm_host && pos_scratch && phi && base && full), "shapley_reduce: finish needs the table, its scratch, phi, base and "
            "full");
  if (finish)
    if (int rc = upload_positions("shapley_reduce", perm_host, P, M, pos_scratch, stream)) return rc;
  const int K = 2 * P * (M - 1);
  const int64_t coalitions = coalition_rows / G;
  auto unit_of = [&](int64_t r) { return r >= coalition_rows ? coalitions + (r - coalition_rows) : r / G; };
  const int64_t unit0 = unit_of(row0), n_units = unit_of(row1) - unit0;
  if (n_units > 0) {
    int cpad = 2;
    while (cpad < C) cpad <<= 1;
    const dim3 grid((unsigned)((n_units + NT / 64 - 1) / (NT / 64)));
    if (logits_dtype == 1)
      hipLaunchKernelGGL(shapley_value_kernel<bf16_t>, grid, dim3(NT), 0, ST(stream), (const bf16_t*)logits, C, cpad, G, K, output, row0, unit0,
                         n_units, coalitions, v);
    else
      hipLaunchKernelGGL(shapley_value_kernel<float>, grid, dim3(NT), 0, ST(stream), (const float*)logits, C, cpad, G, K, output, row0, unit0,
                         n_units, coalitions, v);
    HIP_CHECK_RET(hipGetLastError());
  }
  if (finish) {
    const int64_t total = (int64_t)batch * M * C;
    hipLaunchKernelGGL(shapley_phi_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ST(stream), v, pos_scratch, batch, P, M, C, phi,
                       base, full);
    HIP_CHECK_RET(hipGetLastError());
    if (abs_sum) {
      hipLaunchKernelGGL(shapley_accumulate_kernel, dim3(ceil_div(M * C, NT)), dim3(NT), 0, ST(stream), phi, batch, M * C, abs_sum);
      HIP_CHECK_RET(hipGetLastError());
    }
  }
  return MMSKIN_OK;
}
