// Rectangular linear sum assignment on the DEVICE: every (layer x image) Hungarian problem of a training step in one launch,
// with the indices of csrc/lsap.hip (and therefore of scipy.optimize.linear_sum_assignment), so that the step needs no
// device -> host copy of the cost matrices and no host solve (mask2former_head._targets_batched).
//
// Work split: ONE wavefront per problem (one workgroup of 64 lanes). The algorithm is a few hundred strictly sequential
// iterations around an argmin over at most max(nr, nc) columns; more waves per problem would put a cross-wave barrier into each
// of them, and the 160 problems of configs[2] fill 160 CUs once anyway.
//
// Arithmetic: `lsap_solve` of csrc/lsap.hip. Costs are f32 widened to f64 (exact), u / v / dist / min_val are f64 and the
// reduced cost is ((min_val + c) - u[i]) - v[j]: adds only, nothing to contract, so every dist is the host solver's bit for bit.
// nc < nr is solved on the transpose, as there. The (transposed) matrix is staged ONCE into LDS as f32: the source is read
// coalesced in its row-major order and written transposed, so the usual G < Q case does not read a strided column per iteration.
//
// The column scan is the one parallel part. Columns are owned by their POSITION `it` in remaining[0 .. n_rem), strided over the
// lanes; each lane updates dist / path of its columns; the winner is the minimum dist of the wave and, among the positions that
// hold it, the LARGEST position whose column is unassigned if there is one, else the SMALLEST position. That is what the
// sequential scan's `dist < lowest || (dist == lowest && row4col[j] == -1)` selects (the first minimum stands until an
// unassigned column of the same dist replaces it, and every later such column replaces that one). One lane then does the
// host code's swap-remove remaining[index] = remaining[--n_rem], so later scans walk the same permutation. The rule is written
// down in numpy as `assigner.lsap_wave_rule_host`.
//
// Bad input neither faults nor hangs: NaN / -inf seen while staging -> status 1 ("invalid numeric entries"), a scan whose
// minimum is +inf -> status 2 ("infeasible"), a descriptor that does not fit the buffers or the launch's LDS -> status 3 (nothing
// written); every loop is bounded by nr / nc. A problem with status 1 / 2 writes the identity pairing k -> (k, k), which is in
// range for every consumer; the two status words keep [code, problem + 1] of the first (lowest-index) failure.
#include "cgg_common.h"

#define LSAP_DESC 6          // int64 words per problem: cost offset, nr, nc, output offset, label-row offset, gt-label offset
#define LSAP_MAX_SIDE CGG_LSAP_MAX_SIDE

namespace {

// [code, problem + 1] as ONE 64-bit word (code in the low half), kept for the LOWEST failing problem index whatever order the
// workgroups run in: a vector compare-and-swap, repeated only while a higher index holds the word.
__device__ inline void lsap_report(int* status, int code, int p) {
  unsigned long long* s = reinterpret_cast<unsigned long long*>(status);
  const unsigned long long mine = ((unsigned long long)(unsigned)(p + 1) << 32) | (unsigned)code;
  unsigned long long old = atomicCAS(s, 0ull, mine);
  while (old != 0ull && old > mine) {
    const unsigned long long prev = atomicCAS(s, old, mine);
    if (prev == old) break;
    old = prev;
  }
}

__host__ __device__ inline long long lsap_lds_bytes(long long nr, long long nc) {
  const long long R = nr < nc ? nr : nc, C = nr < nc ? nc : nr;
  // u[R] f64 | v[C], dist[C] f64 | cost[R * C] f32 | path, row4col, remaining [C] i32 | col4row[R] i32 | SR[R], SC[C] bytes
  const long long b = 8 * R + 16 * C + 4 * R * C + 12 * C + 4 * R + R + C;
  return (b + 15) & ~15ll;
}

__global__ __launch_bounds__(64) void cgg_lsap_device_kernel(const float* __restrict__ cost, const int64_t* __restrict__ desc,
                                                            long long cost_numel, long long out_numel, long long rows_numel,
                                                            long long gt_numel, long long lds_bytes, int64_t* __restrict__ q_out,
                                                            int64_t* __restrict__ g_out, const int64_t* __restrict__ gt_labels,
                                                            int64_t* __restrict__ labels, float* __restrict__ weights,
                                                            int* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char lsap_smem[];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int64_t* d = desc + (size_t)p * LSAP_DESC;
  const long long coff = d[0], nr_ = d[1], nc_ = d[2], ooff = d[3], roff = d[4], loff = d[5];
  const bool epilogue = labels != nullptr;
  bool bad = nr_ < 1 || nc_ < 1 || nr_ > LSAP_MAX_SIDE || nc_ > LSAP_MAX_SIDE || coff < 0 || ooff < 0;
  if (!bad) {
    const long long m = nr_ < nc_ ? nr_ : nc_;
    bad = lsap_lds_bytes(nr_, nc_) > lds_bytes || coff + nr_ * nc_ > cost_numel || ooff + m > out_numel;
    if (!bad && epilogue) bad = roff < 0 || loff < 0 || roff + nr_ > rows_numel || loff + nc_ > gt_numel;
  }
  if (bad) {      // (uniform over the workgroup: every lane read the same descriptor)
    if (lane == 0) lsap_report(status, 3, p);
    return;
  }
  const int nr = (int)nr_, nc = (int)nc_;
  const bool transpose = nc < nr;
  const int R = transpose ? nc : nr, C = transpose ? nr : nc;

  double* u = reinterpret_cast<double*>(lsap_smem);
  double* v = u + R;
  double* dist = v + C;
  float* cs = reinterpret_cast<float*>(dist + C);
  int* path = reinterpret_cast<int*>(cs + (size_t)R * C);
  int* row4col = path + C;
  int* remaining = row4col + C;
  int* col4row = remaining + C;
  unsigned char* SR = reinterpret_cast<unsigned char*>(col4row + R);
  unsigned char* SC = SR + R;

  const double INF = __builtin_huge_val();
  int fail = 0;
  {
    // stage: coalesced reads of the row-major nr x nc source, transposed writes when the transpose is solved
    const float* src = cost + coff;
    const int total = nr * nc;
    int invalid = 0;
    for (int t = lane; t < total; t += CGG_WAVE) {
      const float x = src[t];
      if (x != x || x == -__builtin_huge_valf()) invalid = 1;
      if (transpose) {
        const int i = t / nc, j = t - i * nc;
        cs[j * nr + i] = x;
      } else {
        cs[t] = x;
      }
    }
    for (int r = lane; r < R; r += CGG_WAVE) {
      u[r] = 0.0;
      col4row[r] = -1;
    }
    for (int j = lane; j < C; j += CGG_WAVE) {
      v[j] = 0.0;
      row4col[j] = -1;
      path[j] = -1;
    }
    if (__syncthreads_or(invalid)) fail = 1;
  }

  for (int cur = 0; cur < R && !fail; ++cur) {
    // shortest augmenting path from row `cur` to any unassigned column
    for (int j = lane; j < C; j += CGG_WAVE) {
      remaining[j] = C - j - 1;
      dist[j] = INF;
      SC[j] = 0;
    }
    for (int r = lane; r < R; r += CGG_WAVE) SR[r] = 0;
    __syncthreads();
    double min_val = 0.0;
    int n_rem = C, sink = -1, i = cur;
    for (int step = 0; step < C && sink == -1; ++step) {
      const double ui = u[i];
      const float* ci = cs + (size_t)i * C;
      double best = INF;
      int tie = 0x7fffffff;       // C - 1 - it for an unassigned column, C + it otherwise: the smaller wins among equal dist
      for (int it = lane; it < n_rem; it += CGG_WAVE) {
        const int j = remaining[it];
        const double r = min_val + (double)ci[j] - ui - v[j];
        double dj = dist[j];
        if (r < dj) {
          path[j] = i;
          dist[j] = r;
          dj = r;
        }
        const int t = row4col[j] == -1 ? C - 1 - it : C + it;
        if (dj < best || (dj == best && t < tie)) {
          best = dj;
          tie = t;
        }
      }
#pragma unroll
      for (int off = CGG_WAVE / 2; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int ot = __shfl_xor(tie, off);
        if (ob < best || (ob == best && ot < tie)) {
          best = ob;
          tie = ot;
        }
      }
      if (lane == 0) SR[i] = 1;
      min_val = best;
      if (!(best < INF)) {        // infeasible (wave-uniform: every lane holds the reduced pair)
        fail = 2;
        break;
      }
      const int index = tie < C ? C - 1 - tie : tie - C;
      const int j = remaining[index];
      const int rj = row4col[j];
      __syncthreads();            // every lane has read remaining[index] before it is overwritten
      if (lane == 0) {
        SC[j] = 1;
        remaining[index] = remaining[n_rem - 1];
      }
      --n_rem;
      if (rj == -1) sink = j;
      else i = rj;
      __syncthreads();            // dist / path / remaining of this scan are visible to the next one's owners
    }
    if (!fail && sink == -1) fail = 2;
    if (fail) break;
    // dual update (each entry is independent: the host code's values)
    for (int r = lane; r < R; r += CGG_WAVE) {
      const int cj = col4row[r];         // (a visited row other than `cur` is an assigned one)
      if (SR[r] && (r == cur || cj >= 0)) u[r] += r == cur ? min_val : min_val - dist[cj];
    }
    for (int j = lane; j < C; j += CGG_WAVE)
      if (SC[j]) v[j] -= min_val - dist[j];
    __syncthreads();
    // augment along the path
    if (lane == 0) {
      int j = sink;
      for (int s = 0; s <= R && j >= 0; ++s) {
        const int r = path[j];
        if (r < 0) break;
        row4col[j] = r;
        const int t = col4row[r];
        col4row[r] = j;
        j = t;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }

  // pairs in scipy's order (rows ascending); solved on the transpose, col4row[g] is the query of ground truth g and the pairs
  // are ranked by query
  for (int k = lane; k < R; k += CGG_WAVE) {
    int q, g, at;
    if (fail) {
      q = g = at = k;
    } else if (!transpose) {
      q = at = k;
      g = col4row[k];
    } else {
      g = k;
      q = col4row[k];
      at = 0;
      for (int k2 = 0; k2 < R; ++k2) at += col4row[k2] < q ? 1 : 0;
    }
    if ((unsigned)q >= (unsigned)nr || (unsigned)g >= (unsigned)nc) q = g = at = k;      // never out of a consumer's range
    q_out[ooff + at] = q;
    g_out[ooff + at] = g;
    if (epilogue) {
      labels[roff + q] = gt_labels[loff + g];
      weights[roff + q] = 1.0f;
    }
  }
  if (fail && lane == 0) lsap_report(status, fail, p);
}

}  // namespace

extern "C" int64_t cgg_lsap_device_lds_bytes(int nr, int nc) {
  if (nr < 1 || nc < 1) return 0;
  return lsap_lds_bytes(nr, nc);
}

// desc: n_problems x 6 int64 on the device (cost offset, nr, nc, output offset, label-row offset, gt-label offset; offsets in
// elements). lds_bytes: the largest cgg_lsap_device_lds_bytes(nr, nc) of the table (a host number: the table is not read here).
extern "C" int cgg_lsap_device_f32(const float* cost, int64_t cost_numel, const int64_t* desc, int n_problems, int64_t lds_bytes,
                                   int64_t* q_out, int64_t* g_out, int64_t out_numel, const int64_t* gt_labels,
                                   int64_t gt_numel, int64_t* labels, float* weights, int64_t rows_numel, int32_t* status,
                                   cgg_stream_t stream) {
  CGG_REQUIRE(n_problems >= 0, CGG_EINVAL, "cgg_lsap_device_f32: n_problems = %d", n_problems);
  if (n_problems == 0) return CGG_OK;
  CGG_REQUIRE(cost && desc && q_out && g_out && status, CGG_EINVAL, "cgg_lsap_device_f32: null pointer");
  CGG_REQUIRE((((uintptr_t)status) & 7u) == 0, CGG_EINVAL, "cgg_lsap_device_f32: status must be 8-byte aligned");
  CGG_REQUIRE((gt_labels != nullptr) == (labels != nullptr) && (labels != nullptr) == (weights != nullptr), CGG_EINVAL,
              "cgg_lsap_device_f32: the epilogue needs gt_labels, labels and weights together");
  CGG_REQUIRE(cost_numel >= 0 && out_numel >= 0 && gt_numel >= 0 && rows_numel >= 0, CGG_EINVAL,
              "cgg_lsap_device_f32: negative buffer size");
  const int64_t limit = cgg_dynamic_lds_limit();
  CGG_REQUIRE(lds_bytes > 0 && lds_bytes <= limit, CGG_EUNSUPPORTED,
              "cgg_lsap_device_f32: %lld bytes of LDS per problem (the device allows %lld)", (long long)lds_bytes, (long long)limit);
  CGG_RAISE_LDS(cgg_lsap_device_kernel, (size_t)lds_bytes, "cgg_lsap_device_f32");
  hipLaunchKernelGGL(cgg_lsap_device_kernel, dim3(n_problems), dim3(CGG_WAVE), (size_t)lds_bytes, (hipStream_t)stream, cost, desc,
                     (long long)cost_numel, (long long)out_numel, (long long)rows_numel, (long long)gt_numel, (long long)lds_bytes, q_out, g_out, gt_labels, labels, weights, status);
  CGG_CHECK_LAUNCH("cgg_lsap_device_f32");
  return CGG_OK;
}
