// One step of the caption beam search for a whole batch of images, on the device: the loop body of the reference's beam_search
// (open_set/utils/eval/inference.py:113-149), which the reference and caption_search.beam_search run on the host for one image.
// The rule -- quirks included -- is written down in caption_search.py (`beam_step_host`); this file follows it:
//   mean over the L decoder blocks' generator outputs -> log-softmax per live row -> (log p + weight[row]) / length^alpha ->
//   the `beam` largest over an image's live rows, descending, equal values by the smaller row * V + col -> de-normalise ->
//   walk: EOS finishes a sequence (score w / (length + 1)^alpha, running best reset every step, stop at `beam` finished), any other
//   token continues it while length + 1 < max_len - 1 and inherits w[parent row] (sic); nothing continued = the image is done.
//
// Pass 1, grid (chunk, slot, image), 256 threads: a workgroup reads BS_CHUNK columns of its row from each of the L blocks once (8-byte
// loads where the rows are 8-byte aligned -- 30 522 * 4 bytes is a multiple of 8 and not of 16 -- scalar loads otherwise), forms the
// mean in registers and writes one record: the chunk's maximum, its sum of exp(x - max), and its `beam` largest means with their
// columns. Inside a row the order by `weighted` is the order by logit, so nothing outside a row's top `beam` can be selected and the
// nlive * V top-k is never formed. Rows of dead slots and of done images exit at once.
// Pass 2, one workgroup per image: log-sum-exp per row from the records, `weighted` for the nlive * chunks * beam survivors, `beam`
// rounds of arg-max in rule order (each round takes the best candidate strictly after the previous winner, so no candidate list is
// kept), then lane 0 walks the winners and plans the new state; the sequences are re-gathered by parent from an LDS copy of the old
// ones, because parent rows overlap. The partials travel between two plain launches.
#include <limits.h>
#include <math.h>

#include "cgg_common.h"

#define BS_THREADS 256
#define BS_CHUNK 1024 /* columns per workgroup of pass 1: 30 chunks x 14 rows = 420 workgroups at V = 30 522, two images */
#define BS_SLOTS CGG_BEAM_STEP_MAX_BEAM
#define BS_REC (2 + 2 * BS_SLOTS) /* words per (row, chunk) record: max, sum exp, BS_SLOTS values, BS_SLOTS columns (-1 = none) */

// rule order: larger value first, equal values by the smaller key
__device__ __forceinline__ bool bs_before(float v1, int k1, float v2, int k2) { return v1 > v2 || (v1 == v2 && k1 < k2); }

// the first of the workgroup's (v, k) in rule order, for every thread; `slot` alternates between calls so that one barrier is enough
__device__ __forceinline__ void bs_block_first(float& v, int& k, float (*sv)[BS_THREADS / CGG_WAVE], int (*sk)[BS_THREADS / CGG_WAVE],
                                               int slot) {
#pragma unroll
  for (int o = CGG_WAVE / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, CGG_WAVE);
    const int ok = __shfl_xor(k, o, CGG_WAVE);
    if (bs_before(ov, ok, v, k)) {
      v = ov;
      k = ok;
    }
  }
  if ((threadIdx.x & (CGG_WAVE - 1)) == 0) {
    sv[slot][threadIdx.x / CGG_WAVE] = v;
    sk[slot][threadIdx.x / CGG_WAVE] = k;
  }
  __syncthreads();
  v = sv[slot][0];
  k = sk[slot][0];
#pragma unroll
  for (int w = 1; w < BS_THREADS / CGG_WAVE; ++w)
    if (bs_before(sv[slot][w], sk[slot][w], v, k)) {
      v = sv[slot][w];
      k = sk[slot][w];
    }
}

__global__ __launch_bounds__(BS_THREADS) void cgg_beam_partials_kernel(const float* __restrict__ logits, int L, int S, int V,
                                                                       int nchunk, const int32_t* __restrict__ nlive,
                                                                       const int32_t* __restrict__ done, float* __restrict__ ws,
                                                                       int vec2) {
  __shared__ float sv[2][BS_THREADS / CGG_WAVE];
  __shared__ int sk[2][BS_THREADS / CGG_WAVE];
  __shared__ float ssum[BS_THREADS / CGG_WAVE];
  const int chunk = blockIdx.x, s = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  if (done[b] != 0 || s >= nlive[b]) return;   // workgroup-uniform
  const size_t rows = (size_t)gridDim.z * S, row = (size_t)b * S + s;
  const int c0 = chunk * BS_CHUNK;

  // this thread's 4 columns: two adjacent pairs, 512 columns apart (a wavefront's 8-byte loads cover 512 contiguous bytes)
  float x[4] = {0.f, 0.f, 0.f, 0.f};
  int col[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    col[2 * j] = c0 + j * (BS_CHUNK / 2) + 2 * tid;
    col[2 * j + 1] = col[2 * j] + 1;
  }
  for (int l = 0; l < L; ++l) {
    const float* p = logits + ((size_t)l * rows + row) * V;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = col[2 * j];
      if (vec2 && c + 1 < V) {                   // V even and the base 8-byte aligned: every even column is 8-byte aligned
        const float2 t = *reinterpret_cast<const float2*>(p + c);
        x[2 * j] += t.x;
        x[2 * j + 1] += t.y;
      } else {
        if (c < V) x[2 * j] += p[c];
        if (c + 1 < V) x[2 * j + 1] += p[c + 1];
      }
    }
  }
  const float fl = (float)L;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (col[i] < V) {
      x[i] = x[i] / fl;
    } else {
      x[i] = -INFINITY;
      col[i] = INT_MAX;
    }
  }

  // the chunk's maximum and sum of exp(x - max)
  float m = -INFINITY;
  int mk = INT_MAX;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (bs_before(x[i], col[i], m, mk)) {
      m = x[i];
      mk = col[i];
    }
  float top = m;
  int topk = mk;
  bs_block_first(top, topk, sv, sk, 0);          // round 0 of the selection as well: the first in rule order holds the maximum
  const float cmax = top;
  float e = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (col[i] != INT_MAX && x[i] != -INFINITY) e += expf(x[i] - cmax);
#pragma unroll
  for (int o = CGG_WAVE / 2; o > 0; o >>= 1) e += __shfl_xor(e, o, CGG_WAVE);
  if ((tid & (CGG_WAVE - 1)) == 0) ssum[tid / CGG_WAVE] = e;

  float* rec = ws + (row * nchunk + chunk) * BS_REC;
  int* reci = reinterpret_cast<int*>(rec);
  unsigned taken = 0;
  for (int r = 0; r < BS_SLOTS; ++r) {
    if (r > 0) {
      top = -INFINITY;
      topk = INT_MAX;
      if (r < S) {                               // uniform: S is the beam width
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (!(taken & (1u << i)) && bs_before(x[i], col[i], top, topk)) {
            top = x[i];
            topk = col[i];
          }
        bs_block_first(top, topk, sv, sk, r & 1);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (col[i] == topk && topk != INT_MAX) taken |= 1u << i;
    if (tid == 0) {
      rec[2 + r] = top;
      reci[2 + BS_SLOTS + r] = topk == INT_MAX ? -1 : topk;
    }
  }
  __syncthreads();                               // ssum
  if (tid == 0) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < BS_THREADS / CGG_WAVE; ++w) t += ssum[w];
    rec[0] = cmax;
    rec[1] = t;
  }
}

struct BsArgs {
  const float* ws;
  int32_t* seqs;
  float* weights;
  int32_t* nlive;
  int32_t* fin_seqs;
  int32_t* fin_len;
  float* fin_score;
  int32_t* nfin;
  int32_t* best_idx;
  int32_t* done;
  int32_t* ndone;
  int64_t* tokens;
  int64_t* parents;
  int S, V, nchunk, length, eos, max_len, ML, first;
  float lenpow, lenpow1;   // length^alpha, (length + 1)^alpha
};

__global__ __launch_bounds__(BS_THREADS) void cgg_beam_decide_kernel(BsArgs a) {
  __shared__ int32_t old[BS_SLOTS * CGG_BEAM_STEP_MAX_LEN];
  __shared__ float sv[2][BS_THREADS / CGG_WAVE];
  __shared__ int sk[2][BS_THREADS / CGG_WAVE];
  __shared__ float lse[BS_SLOTS], wrow[BS_SLOTS], selw[BS_SLOTS];
  __shared__ int selkey[BS_SLOTS], plan_parent[BS_SLOTS], plan_col[BS_SLOTS], fplan_row[BS_SLOTS], fplan_col[BS_SLOTS];
  __shared__ int s_nnew, s_nfin_old, s_nfin_new, s_done;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (CGG_WAVE - 1), wave = tid / CGG_WAVE;
  const int S = a.S, V = a.V, ML = a.ML, len = a.length;
  if (a.done[b] != 0) {                          // untouched, but the decoder still needs valid rows to run
    if (tid < S) {
      a.tokens[b * S + tid] = a.eos;
      a.parents[b * S + tid] = b * S + tid;
    }
    return;
  }
  const int nl = min(max(a.nlive[b], 0), S);
  for (int i = tid; i < nl * ML; i += BS_THREADS) old[i] = a.seqs[(size_t)b * S * ML + i];
  if (tid < BS_SLOTS) {
    selw[tid] = 0.f;
    selkey[tid] = INT_MAX;
    wrow[tid] = tid < nl ? a.weights[b * S + tid] : 0.f;
  }
  // log-sum-exp of each live row from its chunks' (max, sum) pairs: one wavefront per row
  for (int r = wave; r < nl; r += BS_THREADS / CGG_WAVE) {
    const float* rec = a.ws + ((size_t)(b * S + r) * a.nchunk) * BS_REC;
    float m = -INFINITY;
    for (int c = lane; c < a.nchunk; c += CGG_WAVE) m = fmaxf(m, rec[(size_t)c * BS_REC]);
#pragma unroll
    for (int o = CGG_WAVE / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, CGG_WAVE));
    float t = 0.f;
    for (int c = lane; c < a.nchunk; c += CGG_WAVE) {
      const float cm = rec[(size_t)c * BS_REC];
      if (cm != -INFINITY) t += rec[(size_t)c * BS_REC + 1] * expf(cm - m);
    }
#pragma unroll
    for (int o = CGG_WAVE / 2; o > 0; o >>= 1) t += __shfl_xor(t, o, CGG_WAVE);
    if (lane == 0) lse[r] = m + logf(t);
  }
  __syncthreads();

  // the `beam` first candidates in rule order; round i takes the first one strictly after round i - 1's winner
  const int ncand = nl * a.nchunk * BS_SLOTS, per_row = a.nchunk * BS_SLOTS;
  float pv = INFINITY;
  int pk = -1, found = 0;
  for (int i = 0; i < S; ++i) {
    float bv = -INFINITY;
    int bk = INT_MAX;
    for (int c = tid; c < ncand; c += BS_THREADS) {
      const int r = c / per_row, q = c - r * per_row, ch = q / BS_SLOTS, j = q - ch * BS_SLOTS;
      const float* rec = a.ws + ((size_t)(b * S + r) * a.nchunk + ch) * BS_REC;
      const int col = reinterpret_cast<const int*>(rec)[2 + BS_SLOTS + j];
      if (col < 0) continue;
      const float v = ((rec[2 + j] - lse[r]) + wrow[r]) / a.lenpow;
      const int key = r * V + col;
      if ((v < pv || (v == pv && key > pk)) && bs_before(v, key, bv, bk)) {
        bv = v;
        bk = key;
      }
    }
    bs_block_first(bv, bk, sv, sk, i & 1);
    if (bk == INT_MAX) break;                    // uniform: fewer candidates than `beam` (NaN logits)
    if (tid == 0) {
      selw[i] = bv * a.lenpow;
      selkey[i] = bk;
    }
    pv = bv;
    pk = bk;
    found = i + 1;
  }
  __syncthreads();

  if (tid == 0) {                                // the walk of inference.py:126-143, serial by definition
    int nfin = min(max(a.nfin[b], 0), S), nnew = 0, dn = 0, best = 0;
    const int nfin_old = nfin;
    float best_score = -100.f, neww[BS_SLOTS];
    for (int i = 0; i < found; ++i) {
      const int row = selkey[i] / V, col = selkey[i] - row * V;
      if (a.first) {
        neww[nnew] = selw[i];
        plan_parent[nnew] = row;
        plan_col[nnew] = col;
        ++nnew;
      } else if (col == a.eos) {
        if (nfin >= S) {
          dn = 1;
          break;
        }
        const float score = selw[i] / a.lenpow1;
        fplan_row[nfin - nfin_old] = row;
        fplan_col[nfin - nfin_old] = col;
        a.fin_score[b * S + nfin] = score;
        a.fin_len[b * S + nfin] = len + 1;
        if (score > best_score) {
          best_score = score;
          best = nfin;
        }
        ++nfin;
        if (nfin == S) {
          dn = 1;
          break;
        }
      } else if (len + 1 < a.max_len - 1) {
        neww[nnew] = selw[row];                  // (sic) the new weights indexed by the parent row
        plan_parent[nnew] = row;
        plan_col[nnew] = col;
        ++nnew;
      }
    }
    if (nnew == 0) {
      dn = 1;
    } else {
      for (int n = 0; n < nnew; ++n) a.weights[b * S + n] = neww[n];
      a.nlive[b] = nnew;
    }
    if (!a.first) a.best_idx[b] = best;
    a.nfin[b] = nfin;
    if (dn) {
      a.done[b] = 1;
      atomicAdd(a.ndone, 1);
    }
    s_nnew = nnew;
    s_nfin_old = nfin_old;
    s_nfin_new = nfin;
    s_done = dn;
  }
  __syncthreads();

  const int nnew = s_nnew, nf0 = s_nfin_old, nf1 = s_nfin_new;
  for (int i = tid; i < (nf1 - nf0) * (len + 1); i += BS_THREADS) {
    const int f = i / (len + 1), t = i - f * (len + 1);
    a.fin_seqs[((size_t)b * S + nf0 + f) * ML + t] = t < len ? old[fplan_row[f] * ML + t] : fplan_col[f];
  }
  for (int i = tid; i < nnew * (len + 1); i += BS_THREADS) {
    const int n = i / (len + 1), t = i - n * (len + 1);
    a.seqs[((size_t)b * S + n) * ML + t] = t < len ? old[plan_parent[n] * ML + t] : plan_col[n];
  }
  if (tid < S) {
    const bool live = !s_done && tid < nnew;
    a.tokens[b * S + tid] = live ? plan_col[tid] : a.eos;
    a.parents[b * S + tid] = b * S + (live ? plan_parent[tid] : tid);
  }
}

static int bs_chunks(int V) { return (V + BS_CHUNK - 1) / BS_CHUNK; }

extern "C" int64_t cgg_beam_step_workspace_bytes(int B, int beam, int V) {
  if (B < 1 || beam < 1 || V < 1) return 0;
  return (int64_t)B * beam * bs_chunks(V) * BS_REC * 4;
}

extern "C" int cgg_beam_step_passes(const float* logits, int L, int B, int beam, int V, int32_t* seqs, float* weights, int32_t* nlive,
                                    int32_t* fin_seqs, int32_t* fin_len, float* fin_score, int32_t* nfin, int32_t* best_idx,
                                    int32_t* done, int32_t* ndone, int64_t* tokens, int64_t* parents, void* ws, int length,
                                    float alpha, int eos, int max_len, int state_max_len, int first, int passes,
                                    cgg_stream_t stream) {
  const char* me = "cgg_beam_step";
  CGG_REQUIRE(logits && seqs && weights && nlive && fin_seqs && fin_len && fin_score && nfin && best_idx && done && ndone && tokens &&
                  parents && ws,
              CGG_EINVAL, "%s: null pointer", me);
  CGG_REQUIRE(L >= 1 && B >= 1, CGG_EINVAL, "%s: L and B must be >= 1 (got %d, %d)", me, L, B);
  CGG_REQUIRE(beam >= 1 && beam <= CGG_BEAM_STEP_MAX_BEAM, CGG_EINVAL, "%s: beam must be in 1 .. %d (got %d)", me,
              CGG_BEAM_STEP_MAX_BEAM, beam);
  CGG_REQUIRE(V >= beam, CGG_EINVAL, "%s: V = %d is smaller than beam = %d", me, V, beam);
  CGG_REQUIRE(state_max_len >= 2 && max_len <= state_max_len, CGG_EINVAL,
              "%s: max_len = %d is larger than the %d tokens the state was sized for", me, max_len, state_max_len);
  CGG_REQUIRE(length >= 1 && length < state_max_len, CGG_EINVAL, "%s: length must be in 1 .. state_max_len - 1 = %d (got %d)", me,
              state_max_len - 1, length);
  CGG_REQUIRE(passes >= 1 && passes <= 3, CGG_EINVAL, "%s: passes must be 1, 2 or 3 (got %d)", me, passes);
  CGG_REQUIRE(alpha == alpha, CGG_EINVAL, "%s: alpha is not a number", me);
  CGG_REQUIRE(state_max_len <= CGG_BEAM_STEP_MAX_LEN, CGG_EUNSUPPORTED, "%s: state_max_len must be <= %d (got %d)", me,
              CGG_BEAM_STEP_MAX_LEN, state_max_len);
  // keys are row * V + col in int, the grid's z is the image
  CGG_REQUIRE(V < (1 << 27) && B <= 65535, CGG_EUNSUPPORTED, "%s: V must be < 2^27 and B <= 65535 (got %d, %d)", me, V, B);
  CGG_REQUIRE((((uintptr_t)logits) & 3u) == 0, CGG_EALIGN, "%s: logits must be 4-byte aligned", me);
  const int nchunk = bs_chunks(V);
  if (passes & 1) {
    const int vec2 = (V % 2 == 0) && ((((uintptr_t)logits) & 7u) == 0);
    hipLaunchKernelGGL(cgg_beam_partials_kernel, dim3((unsigned)nchunk, (unsigned)beam, (unsigned)B), dim3(BS_THREADS), 0,
                       (hipStream_t)stream, logits, L, beam, V, nchunk, nlive, done, (float*)ws, vec2);
    CGG_CHECK_LAUNCH(me);
  }
  if (passes & 2) {
    BsArgs a;
    a.ws = (const float*)ws;
    a.seqs = seqs;
    a.weights = weights;
    a.nlive = nlive;
    a.fin_seqs = fin_seqs;
    a.fin_len = fin_len;
    a.fin_score = fin_score;
    a.nfin = nfin;
    a.best_idx = best_idx;
    a.done = done;
    a.ndone = ndone;
    a.tokens = tokens;
    a.parents = parents;
    a.S = beam;
    a.V = V;
    a.nchunk = nchunk;
    a.length = length;
    a.eos = eos;
    a.max_len = max_len;
    a.ML = state_max_len;
    a.first = first ? 1 : 0;
    a.lenpow = (float)pow((double)length, (double)alpha);
    a.lenpow1 = (float)pow((double)length + 1.0, (double)alpha);
    hipLaunchKernelGGL(cgg_beam_decide_kernel, dim3((unsigned)B), dim3(BS_THREADS), 0, (hipStream_t)stream, a);
    CGG_CHECK_LAUNCH(me);
  }
  return CGG_OK;
}

extern "C" int cgg_beam_step(const float* logits, int L, int B, int beam, int V, int32_t* seqs, float* weights, int32_t* nlive,
                             int32_t* fin_seqs, int32_t* fin_len, float* fin_score, int32_t* nfin, int32_t* best_idx, int32_t* done,
                             int32_t* ndone, int64_t* tokens, int64_t* parents, void* ws, int length, float alpha, int eos,
                             int max_len, int state_max_len, int first, cgg_stream_t stream) {
  return cgg_beam_step_passes(logits, L, B, beam, V, seqs, weights, nlive, fin_seqs, fin_len, fin_score, nfin, best_idx, done, ndone,
                              tokens, parents, ws, length, alpha, eos, max_len, state_max_len, first, 3, stream);
}
