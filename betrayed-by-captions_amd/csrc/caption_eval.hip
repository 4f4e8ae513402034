// Caption metrics (caption_eval.py states the rules in plain Python; the kernels equal them exactly).
//
// One workgroup of ONE wave per image: sentences are a dozen words, the work is integer compares in LDS, and a wave needs no barrier
// hardware to stay in step (the __syncthreads below are free for it). The image's words are staged in LDS once per stream.
//
// Caps, from the LDS layout below and not measured: a sentence of at most CAP_L = 128 tokens, an image of at most CAP_R = 32
// references. Then an image stages at most (32 + 1) * 128 = 4224 words (16.5 KiB), next to
//   cgg_caption_bleu_lcs_kernel   the LCS rows, 129 x 64 uint16, row j of lane l at [j * 64 + l] (16.1 KiB)          -> 33 KiB
//   cgg_caption_ngram_keys_kernel nothing else                                                                        -> 17 KiB
//   cgg_cider_sums_kernel         term counts of one order: 4224 uint16 (8.3 KiB) + 32 x 128 uint16 against refs (8 KiB) -> 33 KiB
// all under the 64 KiB of static LDS, several workgroups per CU. Every kernel checks the image's offsets and the caps ON THE DEVICE
// before it stages anything: an image that fails is marked (-1 / 0 / -1.0) and nothing is read or written out of bounds.
//
//   "same k-gram" is always a position-against-position compare: m = the number of equal words from positions a and b on, up to 4
//   and up to both sentence ends; the k-grams at a and b exist and are equal iff m >= k.
#include "cgg_common.h"

namespace {

constexpr int CAP_L = CGG_CAPTION_MAX_LEN;
constexpr int CAP_R = CGG_CAPTION_MAX_REFS;
constexpr int CAP_WORDS = (CAP_R + 1) * CAP_L;
constexpr int CE_THREADS = 64;
constexpr int CE_MAX_WORDS = 1 << 28;     // keys / gids are [W][4]: their indices stay in int32

// Sentence offsets of image n of one stream into s_off[0 .. ns] (relative to the image's first word) -> ns, or -1 when the image is
// outside the caps or its offsets are not ascending within 0 .. W. Every lane returns the same value. s_bad: one LDS word.
__device__ __forceinline__ int ce_load_offsets(const int32_t* __restrict__ sent_off, const int32_t* __restrict__ img_off, int n, int S, int W,
                                               int32_t* s_off, int32_t* s_bad, int32_t* base_out) {
  const int s0 = img_off[n], s1 = img_off[n + 1];
  const int ns = s1 - s0;
  if (s0 < 0 || ns < 1 || ns > CAP_R + 1 || s1 > S) return -1;
  const int base = sent_off[s0];
  if (threadIdx.x == 0) *s_bad = (base < 0) ? 1 : 0;
  __syncthreads();
  for (int t = threadIdx.x; t <= ns; t += CE_THREADS) {
    const int o = sent_off[s0 + t];
    s_off[t] = o - base;
    const int nxt = t < ns ? sent_off[s0 + t + 1] : o;
    if (o < 0 || o > W || nxt < o || nxt - o > CAP_L) atomicOr(s_bad, 1);
  }
  __syncthreads();
  const int bad = *s_bad;
  __syncthreads();
  *base_out = base;
  return bad ? -1 : ns;
}

__device__ __forceinline__ int ce_match(const int32_t* a, int amax, const int32_t* b, int bmax) {
  int lim = amax < bmax ? amax : bmax;
  lim = lim < 4 ? lim : 4;
  int m = 0;
  while (m < lim && a[m] == b[m]) ++m;
  return m;
}

__global__ __launch_bounds__(CE_THREADS) void cgg_caption_bleu_lcs_kernel(
    const int32_t* __restrict__ words, const int32_t* __restrict__ sent_off, int W, const int32_t* __restrict__ words_sp,
    const int32_t* __restrict__ sent_off_sp, int W_sp, const int32_t* __restrict__ img_off, int N, int S, int32_t* __restrict__ bleu,
    int32_t* __restrict__ lcs) {
  __shared__ int32_t s_words[CAP_WORDS];
  __shared__ uint16_t s_dp[(CAP_L + 1) * CE_THREADS];
  __shared__ int32_t s_off[CAP_R + 2];
  __shared__ int32_t s_correct[4];
  __shared__ int32_t s_bad;
  const int n = blockIdx.x, lane = threadIdx.x;
  const int P = S - N;
  int base = 0, base_sp = 0;
  // both streams are checked before anything is written: an image is evaluated whole or marked whole
  const int ns_sp = ce_load_offsets(sent_off_sp, img_off, n, S, W_sp, s_off, &s_bad, &base_sp);
  const int ns = ns_sp < 0 ? -1 : ce_load_offsets(sent_off, img_off, n, S, W, s_off, &s_bad, &base);
  if (ns < 0) {
    if (lane < 10) bleu[n * 10 + lane] = -1;
    const int s0 = img_off[n], s1 = img_off[n + 1];
    if (s0 >= 0 && s0 <= s1 && s1 <= S)
      for (int r = lane; r < s1 - s0 - 1; r += CE_THREADS) {
        const int p = s0 - n + r;
        if (p >= 0 && p < P) lcs[p] = -1;
      }
    return;
  }
  const int R = ns - 1;
  const int s0 = img_off[n];
  // ---- BLEU components, from the split() stream ----
  const int total = s_off[ns];
  for (int t = lane; t < total; t += CE_THREADS) s_words[t] = words[base + t];
  if (lane < 4) s_correct[lane] = 0;
  __syncthreads();
  const int Lh = s_off[1];
  for (int i = lane; i < Lh; i += CE_THREADS) {
    int cnt[4] = {0, 0, 0, 0}, maxc[4] = {0, 0, 0, 0};
    bool first[4] = {true, true, true, true};
    for (int j = 0; j < Lh; ++j) {
      const int m = ce_match(s_words + i, Lh - i, s_words + j, Lh - j);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < m) {
          ++cnt[k];
          if (j < i) first[k] = false;
        }
    }
    for (int r = 1; r <= R; ++r) {
      const int o = s_off[r], Lr = s_off[r + 1] - o;
      int c[4] = {0, 0, 0, 0};
      for (int j = 0; j < Lr; ++j) {
        const int m = ce_match(s_words + i, Lh - i, s_words + o + j, Lr - j);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < m) ++c[k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) maxc[k] = c[k] > maxc[k] ? c[k] : maxc[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)       // cnt[k] > 0 iff the (k + 1)-gram at i exists (it matches itself)
      if (cnt[k] > 0 && first[k]) atomicAdd(&s_correct[k], cnt[k] < maxc[k] ? cnt[k] : maxc[k]);
  }
  __syncthreads();
  if (lane == 0) {
    int best_d = 0, best_l = 0;
    for (int r = 1; r <= R; ++r) {      // min((abs(l - testlen), l))
      const int l = s_off[r + 1] - s_off[r];
      const int d = l > Lh ? l - Lh : Lh - l;
      if (r == 1 || d < best_d || (d == best_d && l < best_l)) {
        best_d = d;
        best_l = l;
      }
    }
    int32_t* o = bleu + n * 10;
    o[0] = Lh;
    o[1] = best_l;
    for (int k = 0; k < 4; ++k) {
      o[2 + k] = Lh - k > 0 ? Lh - k : 0;
      o[6 + k] = s_correct[k];
    }
  }
  __syncthreads();
  // ---- LCS per pair, from the split(" ") stream: lane r owns reference r, its DP row in LDS ----
  ce_load_offsets(sent_off_sp, img_off, n, S, W_sp, s_off, &s_bad, &base_sp);      // (checked above)
  const int total_sp = s_off[ns];
  for (int t = lane; t < total_sp; t += CE_THREADS) s_words[t] = words_sp[base_sp + t];
  __syncthreads();
  const int La = s_off[1];
  for (int r = lane; r < R; r += CE_THREADS) {      // (R <= 32: one pass)
    const int o = s_off[r + 1], Lb = s_off[r + 2] - o;
    uint16_t* row = s_dp + lane;
    for (int j = 0; j <= Lb; ++j) row[j * CE_THREADS] = 0;
    for (int i = 1; i <= La; ++i) {
      const int a = s_words[i - 1];
      int diag = 0, left = 0;           // lengths[i - 1][j - 1], lengths[i][j - 1]
      for (int j = 1; j <= Lb; ++j) {
        const int up = row[j * CE_THREADS];
        const int v = a == s_words[o + j - 1] ? diag + 1 : (up > left ? up : left);
        row[j * CE_THREADS] = (uint16_t)v;
        diag = up;
        left = v;
      }
    }
    const int p = s0 - n + r;
    if (p >= 0 && p < P) lcs[p] = row[Lb * CE_THREADS];
  }
}

__global__ __launch_bounds__(CE_THREADS) void cgg_caption_ngram_keys_kernel(const int32_t* __restrict__ words,
                                                                            const int32_t* __restrict__ sent_off, int W,
                                                                            const int32_t* __restrict__ img_off, int N, int S,
                                                                            int64_t* __restrict__ keys, uint8_t* __restrict__ flags) {
  __shared__ int32_t s_words[CAP_WORDS];
  __shared__ int32_t s_off[CAP_R + 2];
  __shared__ int32_t s_bad;
  const int n = blockIdx.x, lane = threadIdx.x;
  int base = 0;
  const int ns = ce_load_offsets(sent_off, img_off, n, S, W, s_off, &s_bad, &base);
  if (ns < 0) {
    // the words this image claims, as far as the claim can be trusted: between its neighbours' first words, within 0 .. W
    const int s0 = img_off[n], s1 = img_off[n + 1];
    if (s0 >= 0 && s0 <= s1 && s1 <= S) {
      const int b = sent_off[s0], e = sent_off[s1];
      if (b >= 0 && b <= e && e <= W)
        for (int64_t t = (int64_t)b * 4 + lane; t < (int64_t)e * 4; t += CE_THREADS) {
          keys[t] = 0;
          flags[t] = 0;
        }
    }
    return;
  }
  const int total = s_off[ns];
  for (int t = lane; t < total; t += CE_THREADS) s_words[t] = words[base + t];
  __syncthreads();
  for (int r = 0; r < ns; ++r) {
    const int o = s_off[r], L = s_off[r + 1] - o;
    for (int i = lane; i < L; i += CE_THREADS) {
      const int32_t* a = s_words + o + i;
      const int avail = L - i;
      bool first[4];
      int64_t key = 0, kk[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < avail) key |= (int64_t)(a[k] & 0xFFFF) << (16 * k);
        kk[k] = k < avail ? key : 0;
        first[k] = r > 0 && k < avail;
      }
      for (int q = 1; q <= r && (first[0] || first[1] || first[2] || first[3]); ++q) {      // earlier reference positions
        const int oq = s_off[q], Lq = q == r ? i : s_off[q + 1] - oq;      // (of the same sentence: those before i)
        const int Lfull = s_off[q + 1] - oq;
        for (int j = 0; j < Lq; ++j) {
          const int m = ce_match(a, avail, s_words + oq + j, Lfull - j);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < m) first[k] = false;
        }
      }
      const int64_t g = ((int64_t)base + o + i) * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        keys[g + k] = kk[k];
        flags[g + k] = first[k] ? 1 : 0;
      }
    }
  }
}

__global__ __launch_bounds__(CE_THREADS) void cgg_cider_sums_kernel(const int32_t* __restrict__ gids, const int32_t* __restrict__ df, int U,
                                                                    const double* __restrict__ idf_by_df,
                                                                    const int32_t* __restrict__ sent_off, int W,
                                                                    const int32_t* __restrict__ img_off, int N, int S,
                                                                    double* __restrict__ norm2, double* __restrict__ num) {
#pragma clang fp contract(off)
  __shared__ int32_t s_g[CAP_WORDS];
  __shared__ uint16_t s_tf[CAP_WORDS];
  __shared__ uint16_t s_rtf[CAP_R * CAP_L];
  __shared__ int32_t s_off[CAP_R + 2];
  __shared__ int32_t s_bad;
  const int n = blockIdx.x, lane = threadIdx.x;
  const int P = S - N;
  int base = 0;
  const int ns = ce_load_offsets(sent_off, img_off, n, S, W, s_off, &s_bad, &base);
  const int s0 = img_off[n];
  if (ns < 0) {
    const int s1 = img_off[n + 1];
    if (s0 >= 0 && s0 <= s1 && s1 <= S) {
      for (int t = lane; t < (s1 - s0) * 4; t += CE_THREADS) norm2[(int64_t)s0 * 4 + t] = -1.0;
      for (int t = lane; t < (s1 - s0 - 1) * 4; t += CE_THREADS) {
        const int64_t p = (int64_t)(s0 - n) * 4 + t;
        if (p >= 0 && p < (int64_t)P * 4) num[p] = -1.0;
      }
    }
    return;
  }
  const int R = ns - 1;
  const int Lh = s_off[1];
  for (int k = 0; k < 4; ++k) {
    // the ids of this order, -1 where the sentence ends before the n-gram does
    for (int r = 0; r < ns; ++r) {
      const int o = s_off[r], L = s_off[r + 1] - o;
      for (int i = lane; i < L; i += CE_THREADS) {
        int g = -1;
        if (i + k < L) {
          g = gids[((int64_t)base + o + i) * 4 + k];
          if (g < 0 || g >= U) g = 0;
        }
        s_g[o + i] = g;
      }
    }
    __syncthreads();
    // tf at the first occurrence of an n-gram in its sentence, 0 elsewhere
    for (int r = 0; r < ns; ++r) {
      const int o = s_off[r], L = s_off[r + 1] - o;
      for (int i = lane; i < L; i += CE_THREADS) {
        const int g = s_g[o + i];
        int cnt = 0;
        bool first = g >= 0;
        if (first)
          for (int j = 0; j < L; ++j)
            if (s_g[o + j] == g) {
              ++cnt;
              if (j < i) first = false;
            }
        s_tf[o + i] = (uint16_t)(first ? cnt : 0);
      }
    }
    __syncthreads();
    // the count, in every reference, of each distinct hypothesis n-gram
    for (int r = 1; r <= R; ++r) {
      const int o = s_off[r], L = s_off[r + 1] - o;
      for (int i = lane; i < Lh; i += CE_THREADS) {
        int cnt = 0;
        if (s_tf[i]) {
          const int g = s_g[i];
          for (int j = 0; j < L; ++j) cnt += s_g[o + j] == g ? 1 : 0;
        }
        s_rtf[(r - 1) * CAP_L + i] = (uint16_t)cnt;
      }
    }
    __syncthreads();
    // one lane, one chain: the norm of a sentence, or the numerator of a pair, summed in order of first occurrence
    for (int c = lane; c < ns + R; c += CE_THREADS) {
      double acc = 0.0;
      if (c < ns) {
        const int o = s_off[c], L = s_off[c + 1] - o;
        for (int i = 0; i < L; ++i) {
          const int tf = s_tf[o + i];
          if (!tf) continue;
          int d = df[s_g[o + i]];
          if (d < 0 || d > N) d = 0;
          const double v = (double)tf * idf_by_df[d];
          const double sq = v * v;
          acc = acc + sq;
        }
        norm2[((int64_t)s0 + c) * 4 + k] = acc;
      } else {
        const int r = c - ns;       // reference r + 1
        for (int i = 0; i < Lh; ++i) {
          const int tf = s_tf[i];
          if (!tf) continue;
          int d = df[s_g[i]];
          if (d < 0 || d > N) d = 0;
          const double idf = idf_by_df[d];
          const double vh = (double)tf * idf;
          const int rt = s_rtf[r * CAP_L + i];
          const double vr = rt ? (double)rt * idf : 0.0;
          const double mn = vr < vh ? vr : vh;       // Python's min(vh, vr)
          const double pr = mn * vr;
          acc = acc + pr;
        }
        const int64_t p = (int64_t)s0 - n + r;
        if (p >= 0 && p < P) num[p * 4 + k] = acc;
      }
    }
    __syncthreads();
  }
}

int ce_check_sizes(const char* who, int N, int S, int W) {
  CGG_REQUIRE(N >= 0 && S >= N && W >= 0, CGG_EINVAL, "%s: bad sizes (N=%d S=%d W=%d; S >= N: every image has a hypothesis)", who, N, S, W);
  CGG_REQUIRE(W <= CE_MAX_WORDS && S <= CE_MAX_WORDS, CGG_EUNSUPPORTED, "%s: W=%d, S=%d: more than 2^28 words or sentences", who, W, S);
  return CGG_OK;
}

}  // namespace

extern "C" int cgg_caption_bleu_lcs_i32(const int32_t* words, const int32_t* sent_off, int W, const int32_t* words_sp,
                                        const int32_t* sent_off_sp, int W_sp, const int32_t* img_off, int N, int S, int32_t* bleu,
                                        int32_t* lcs, cgg_stream_t stream) {
  const char* who = "cgg_caption_bleu_lcs_i32";
  int rc = ce_check_sizes(who, N, S, W);
  if (rc == CGG_OK) rc = ce_check_sizes(who, N, S, W_sp);
  if (rc != CGG_OK) return rc;
  if (N == 0) return CGG_OK;
  CGG_REQUIRE(sent_off && sent_off_sp && img_off && bleu && (W == 0 || words) && (W_sp == 0 || words_sp) && (S == N || lcs), CGG_EINVAL,
              "%s: null pointer", who);
  hipLaunchKernelGGL(cgg_caption_bleu_lcs_kernel, dim3((unsigned)N), dim3(CE_THREADS), 0, (hipStream_t)stream, words, sent_off, W, words_sp,
                     sent_off_sp, W_sp, img_off, N, S, bleu, lcs);
  CGG_CHECK_LAUNCH(who);
  return CGG_OK;
}

extern "C" int cgg_caption_ngram_keys_i64(const int32_t* words, const int32_t* sent_off, int W, const int32_t* img_off, int N, int S,
                                          int64_t* keys, uint8_t* flags, cgg_stream_t stream) {
  const char* who = "cgg_caption_ngram_keys_i64";
  const int rc = ce_check_sizes(who, N, S, W);
  if (rc != CGG_OK) return rc;
  if (N == 0 || W == 0) return CGG_OK;
  CGG_REQUIRE(words && sent_off && img_off && keys && flags, CGG_EINVAL, "%s: null pointer", who);
  CGG_REQUIRE((((uintptr_t)keys) & 7u) == 0, CGG_EINVAL, "%s: keys must be 8-byte aligned", who);
  hipLaunchKernelGGL(cgg_caption_ngram_keys_kernel, dim3((unsigned)N), dim3(CE_THREADS), 0, (hipStream_t)stream, words, sent_off, W, img_off,
                     N, S, keys, flags);
  CGG_CHECK_LAUNCH(who);
  return CGG_OK;
}

extern "C" int cgg_cider_sums_f64(const int32_t* gids, const int32_t* df, int U, const double* idf_by_df, const int32_t* sent_off, int W,
                                  const int32_t* img_off, int N, int S, double* norm2, double* num, cgg_stream_t stream) {
  const char* who = "cgg_cider_sums_f64";
  const int rc = ce_check_sizes(who, N, S, W);
  if (rc != CGG_OK) return rc;
  CGG_REQUIRE(U >= 0, CGG_EINVAL, "%s: U=%d", who, U);
  if (N == 0) return CGG_OK;
  CGG_REQUIRE(idf_by_df && sent_off && img_off && norm2 && (S == N || num) && (W == 0 || (gids && df && U > 0)), CGG_EINVAL,
              "%s: null pointer (or words without an id table)", who);
  CGG_REQUIRE(((((uintptr_t)norm2) | ((uintptr_t)num) | ((uintptr_t)idf_by_df)) & 7u) == 0, CGG_EINVAL, "%s: doubles must be 8-byte aligned", who);
  hipLaunchKernelGGL(cgg_cider_sums_kernel, dim3((unsigned)N), dim3(CE_THREADS), 0, (hipStream_t)stream, gids, df, U, idf_by_df, sent_off, W,
                     img_off, N, S, norm2, num);
  CGG_CHECK_LAUNCH(who);
  return CGG_OK;
}
