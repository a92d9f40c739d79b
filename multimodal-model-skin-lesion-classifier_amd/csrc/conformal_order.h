// The two rules of a conformal prediction set, stated once for the score pass, the replicate kernel and the apply pass of
// conformal.hip (tests/conformal_oracle.py restates them):
//   the order of a row   class a stands above class b iff p_a > p_b, or p_a == p_b and a < b: descending and stable, a tie goes to
//                        the lower class index.  rank(c) = 1 + the number of classes above c.
//   membership           class c is in the set of row x iff score[x][c] <= qhat[c]; qhat = +inf admits every class.
#pragma once

__host__ __device__ __forceinline__ bool stands_above(double pa, int a, double pb, int b) { return pa > pb || (pa == pb && a < b); }
__host__ __device__ __forceinline__ bool in_set(double score, double qhat) { return score <= qhat; }
