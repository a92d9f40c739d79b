// The pair rule of the one-vs-rest AUC, shared by auc.hip (a whole evaluation pass) and permute.hip (one cell of a permutation
// study): a positive row with score si against a negative row with score v counts 2 for a win and 1 for a tie, so that
// auc = wins2 / (2 pos neg) is the Mann-Whitney statistic with ties at half weight (sklearn's roc_auc_score).  A NaN on either
// side is neither greater nor equal: 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ int32_t auc_wins2(float si, float v) { return si > v ? 2 : (si == v ? 1 : 0); }
