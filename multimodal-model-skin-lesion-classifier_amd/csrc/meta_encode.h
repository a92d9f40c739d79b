// One cell of an encoded metadata row -- OneHotEncoder(handle_unknown='ignore') + fillna(-1) + StandardScaler
// (skinLesionDatasets.py:133-183) -- and the host checks of the encoder's layout, shared by metadata_encode_kernel
// (preprocess.hip), metadata_variants_kernel (sweep.hip) and shapley_coalitions_kernel (shapley.hip).  Each kernel keeps its own
// indexing and its own choice of the raw value (mutation, mask, coalition) and calls these for the cell, so a row of any of them
// equals the output of metadata_encode_kernel bit for bit by construction.
//
// No file-scope pragma here: sweep.hip and shapley.hip compile under `#pragma clang fp contract(off)`, preprocess.hip does not,
// and the cell is the same in both -- a compare, and a subtract followed by a divide, in which nothing can contract.
#pragma once
#include "common.h"

// the column this one-hot slot belongs to (n_cat is a handful: linear scan)
__device__ __forceinline__ int meta_slot_column(int j, int n_cat, const int32_t* col_offset) {
  int col = 0;
  while (col + 1 < n_cat && col_offset[col + 1] <= j) ++col;
  return col;
}

// one-hot slot j of a column whose block starts at `offset`; code < 0: category unseen at fit time -> all zeros
__device__ __forceinline__ float meta_onehot_cell(int code, int j, int offset) { return (code == j - offset) ? 1.f : 0.f; }

// numeric column k: a subtract, then a divide (no multiply-add to contract)
__device__ __forceinline__ float meta_numeric_cell(float x, float mean_k, float scale_k, float nan_fill) {
  if (x != x) x = nan_fill;                                       // pd.to_numeric(errors="coerce").fillna(-1)
  return (x - mean_k) / scale_k;
}

// the encoder's layout as an entry point receives it: the column counts, the one-hot width and the offset table on both sides;
// `what` names the caller in the message
inline int check_meta_layout(const char* what, int n_cat, int n_num, int onehot_width, const int32_t* col_offset,
                             const int32_t* col_offset_host) {
  ARG_CHECK(n_cat >= 0 && n_num >= 0 && n_cat + n_num >= 1 && onehot_width >= n_cat, "%s: bad shape (%d categorical, %d numeric, "
            "one-hot width %d)", what, n_cat, n_num, onehot_width);
  ARG_CHECK(col_offset && col_offset_host, "%s: null argument", what);
  ARG_CHECK(col_offset_host[0] == 0 && col_offset_host[n_cat] == onehot_width, "%s: col_offset must run from 0 to the one-hot "
            "width %d", what, onehot_width);
  for (int c = 0; c < n_cat; ++c) ARG_CHECK(col_offset_host[c + 1] > col_offset_host[c], "%s: column %d has no category", what, c);
  return MMSKIN_OK;
}
