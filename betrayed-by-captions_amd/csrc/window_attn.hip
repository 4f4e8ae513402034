// K6w: fused (shifted-)window multi-head self-attention of the Swin blocks, forward and backward. Per SwinBlock this is everything
// between the qkv linear and the proj linear of [3P] mmdet 2.28 mmdet/models/backbones/swin.py (ShiftWindowMSA.forward ->
// WindowMSA.forward): torch.roll, window partition, the (3, B_, heads, N, D) permute, the (B_, heads, N, N) relative-position bias +
// shifted-window mask, softmax(q k^T scale + bias + mask) v, the transpose back, window reverse and the reverse roll -- and the mirror
// of each in the backward. Here all of the re-ordering is address arithmetic:
//
//   * token (y, x) of the rolled map is token ((y + shift) % Hp, (x + shift) % Wp) of the input rows, windows are ws x ws tiles of the
//     rolled map, and a query's result goes back to the row it was read from;
//   * the bias of pair (i, j) is table[(yi - yj + ws - 1)(2 ws - 1) + xi - xj + ws - 1][head] (the head's column staged in LDS once per
//     workgroup), the shifted-window mask is the reference's additive -100 between tokens whose rolled coordinates carry different
//     three-slice region labels; no N x N tensor is read or written.
//
// Work split: one workgroup = one (window, head), one wavefront per 16 tokens of the window (N = ws^2 <= 144: up to 9 wavefronts).
// Scores are computed TRANSPOSED, S^T = K Q^T on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation): the accumulator of a
// lane then holds, for ITS query i = 16 wave + lane % 16, the keys j = 16 ct + 4 (lane / 16) + r -- exactly the B operand of
// O^T = V^T P^T, so the probabilities never leave the registers and the softmax statistics need two cross-lane steps.
// The contraction slot of a lane (lane / 16) may carry any index as long as A and B agree: d = 8 (lane / 16) + e for the score
// products (two 16-byte loads per operand row), j = 16 ct + 4 (lane / 16) + r for P V.
//
// Backward (P recomputed from qkv and the forward's log-sum-exp rows; delta_i = sum_j P_ij dP_ij, which equals rowsum(dO o O)):
//   pass 1, wavefront owns 16 QUERIES: P^T, dP^T = V dO^T, dS^T = P^T o (dP^T - delta) -> dQ^T = K^T dS^T, and the running sum of dS
//           of the lane's own (i, j) positions over the windows of the workgroup's chunk (the grad_table partial);
//   pass 2, wavefront owns 16 KEYS: the same tiles with the roles swapped (S = Q K^T, lane = key) -> dV^T = dO^T P, dK^T = Q^T dS.
// Every token belongs to one window, so grad_qkv is written with plain stores. grad_table: one N x N partial per (chunk, head) in the
// workspace, folded by a second kernel in a fixed order -- no floating-point atomics, bit-reproducible.
#include "cgg_common.h"

#define WA_LD 36        // LDS row stride in floats (16-byte aligned rows, skewed by 4 banks)
#define WA_TAB 532      // (2 * 12 - 1)^2 = 529 table entries of one head, rounded to 16 bytes

typedef __attribute__((ext_vector_type(4))) int wa_i32x4;

struct WaShape {
  int Hp, Wp, C, heads, ws, shift, N, nwx, nwin;      // nwx windows per row, nwin per image
};

// token n of window `win` (over batch x windows): its row in the input map (-1 past the window), and
// info = (ly (2 ws - 1) + lx) | region label << 16
__device__ __forceinline__ void wa_token(const WaShape& g, int win, int n, int& row, int& info) {
  row = -1;
  info = 0;
  if (n >= g.N) return;
  const int b = win / g.nwin, w = win - b * g.nwin;
  const int wy = w / g.nwx, wx = w - wy * g.nwx;
  const int ly = n / g.ws, lx = n - ly * g.ws;
  const int y = wy * g.ws + ly, x = wx * g.ws + lx;             // rolled coordinates
  int yy = y + g.shift, xx = x + g.shift;
  if (yy >= g.Hp) yy -= g.Hp;
  if (xx >= g.Wp) xx -= g.Wp;
  row = (b * g.Hp + yy) * g.Wp + xx;
  int reg = 0;
  if (g.shift > 0) {
    const int ry = y < g.Hp - g.ws ? 0 : (y < g.Hp - g.shift ? 1 : 2);
    const int rx = x < g.Wp - g.ws ? 0 : (x < g.Wp - g.shift ? 1 : 2);
    reg = ry * 3 + rx;
  }
  info = (ly * (2 * g.ws - 1) + lx) | (reg << 16);
}

#define WA_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// acc += A[16 rows at `ar`, this lane's row][8 kq .. 8 kq + 7] x the lane's 8 B values
__device__ __forceinline__ f32x4 wa_dot8(const float* ar, const f32x4& ba, const f32x4& bb, f32x4 acc) {
  const f32x4 aa = *reinterpret_cast<const f32x4*>(ar), ab = *reinterpret_cast<const f32x4*>(ar + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) acc = WA_MFMA(aa[e], ba[e], acc);
#pragma unroll
  for (int e = 0; e < 4; ++e) acc = WA_MFMA(ab[e], bb[e], acc);
  return acc;
}

template <int NT>
__global__ __launch_bounds__(NT * 64) void cgg_window_attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                                      float* __restrict__ out, float* __restrict__ lse, WaShape g,
                                                                      float scale) {
  constexpr int NTOK = NT * 16, NTHR = NT * 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char wa_smem[];
  float* Ks = reinterpret_cast<float*>(wa_smem);       // [NTOK][WA_LD]
  float* Vs = Ks + NTOK * WA_LD;                       // [NTOK][WA_LD]
  float* tab = Vs + NTOK * WA_LD;                      // [WA_TAB] this head's bias column
  int* rows = reinterpret_cast<int*>(tab + WA_TAB);    // [NTOK]
  int* infos = rows + NTOK;                            // [NTOK]
  const int win = blockIdx.x, h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T1 = 2 * g.ws - 1, T = T1 * T1;
  const size_t C3 = (size_t)3 * g.C;

  for (int t = tid; t < T; t += NTHR) tab[t] = table[(size_t)t * g.heads + h];
  if (tid < NTOK) {
    int row, info;
    wa_token(g, win, tid, row, info);
    rows[tid] = row;
    infos[tid] = info;
  }
  __syncthreads();
  for (int idx = tid; idx < NTOK * 8; idx += NTHR) {
    const int n = idx >> 3, c4 = (idx & 7) * 4;
    const int row = rows[n];
    f32x4 k = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
    if (row >= 0) {
      const float* p = qkv + (size_t)row * C3 + g.C + h * 32 + c4;
      k = *reinterpret_cast<const f32x4*>(p);
      v = *reinterpret_cast<const f32x4*>(p + g.C);
    }
    *reinterpret_cast<f32x4*>(Ks + n * WA_LD + c4) = k;
    *reinterpret_cast<f32x4*>(Vs + n * WA_LD + c4) = v;
  }
  __syncthreads();

  const int nct = (g.N + 15) >> 4;
  if (wave >= nct) return;                              // no barrier below
  const int li = lane & 15, kq = lane >> 4;
  const int i = 16 * wave + li;
  const int ri = rows[i], ii = infos[i];
  const int bi = (ii & 0xffff) + (g.ws - 1) * T1 + g.ws - 1, regi = ii >> 16;
  f32x4 qa = {0.f, 0.f, 0.f, 0.f}, qb = qa;
  if (ri >= 0) {
    const float* p = qkv + (size_t)ri * C3 + h * 32 + 8 * kq;
    qa = *reinterpret_cast<const f32x4*>(p) * scale;
    qb = *reinterpret_cast<const f32x4*>(p + 4) * scale;
  }
  // ---- S^T[j][i] = K[j] . (scale q[i]) ----
  f32x4 acc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ct < nct) acc[ct] = wa_dot8(Ks + (16 * ct + li) * WA_LD + 8 * kq, qa, qb, acc[ct]);
  }
  // ---- + bias + mask, row maximum ----
  float m = -1e30f;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    if (ct < nct) {
      const wa_i32x4 ij = *reinterpret_cast<const wa_i32x4*>(infos + 16 * ct + 4 * kq);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * ct + 4 * kq + r;
        float s = acc[ct][r] + tab[bi - (ij[r] & 0xffff)] + ((ij[r] >> 16) != regi ? -100.f : 0.f);
        if (j >= g.N) s = -1e30f;
        acc[ct][r] = s;
        m = fmaxf(m, s);
      }
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  float sum = 0.f;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    if (ct < nct) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(acc[ct][r] - m);        // keys past the window: exp(-1e30 - m) = 0
        acc[ct][r] = p;
        sum += p;
      }
    }
  }
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  // ---- O^T[d][i] = sum_j V[j][d] P^T[j][i] ----
  f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    if (ct < nct) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* vr = Vs + (16 * ct + 4 * kq + r) * WA_LD + li;
        o0 = WA_MFMA(vr[0], acc[ct][r], o0);
        o1 = WA_MFMA(vr[16], acc[ct][r], o1);
      }
    }
  }
  if (ri >= 0) {
    const float inv = 1.f / sum;
    float* op = out + (size_t)ri * g.C + h * 32 + 4 * kq;
    *reinterpret_cast<f32x4*>(op) = o0 * inv;
    *reinterpret_cast<f32x4*>(op + 16) = o1 * inv;
    if (kq == 0) {
      const int HW = g.Hp * g.Wp, b = ri / HW;
      lse[((size_t)b * g.heads + h) * HW + (ri - b * HW)] = m + __logf(sum);
    }
  }
}

template <int NT>
__global__ __launch_bounds__(NT * 64) void cgg_window_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ table,
                                                                      const float* __restrict__ lse, const float* __restrict__ gout,
                                                                      float* __restrict__ gqkv, float* __restrict__ wsp, WaShape g,
                                                                      float scale, int wpc, int nwtot) {
  constexpr int NTOK = NT * 16, NTHR = NT * 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char wa_smem[];
  float* Qs = reinterpret_cast<float*>(wa_smem);       // [NTOK][WA_LD] scale * q
  float* Ks = Qs + NTOK * WA_LD;
  float* Vs = Ks + NTOK * WA_LD;
  float* Gs = Vs + NTOK * WA_LD;                       // dO
  float* tab = Gs + NTOK * WA_LD;                      // [WA_TAB]
  int* rows = reinterpret_cast<int*>(tab + WA_TAB);    // [NTOK]
  int* infos = rows + NTOK;                            // [NTOK]
  float* Ls = reinterpret_cast<float*>(infos + NTOK);  // [NTOK] log-sum-exp of the window's queries
  float* Ds = Ls + NTOK;                               // [NTOK] delta
  const int chunk = blockIdx.x, h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int T1 = 2 * g.ws - 1, T = T1 * T1;
  const int bconst = (g.ws - 1) * T1 + g.ws - 1;
  const size_t C3 = (size_t)3 * g.C;
  const int HW = g.Hp * g.Wp;
  const int nct = (g.N + 15) >> 4;
  const bool active = wave < nct;
  const int n_own = 16 * wave + li;                     // the query (pass 1) / key (pass 2) of this lane

  for (int t = tid; t < T; t += NTHR) tab[t] = table[(size_t)t * g.heads + h];

  f32x4 tsum[NT];                                       // sum over the chunk's windows of dS[i = n_own][j = 16 ct + 4 kq + r]
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) tsum[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int w0 = chunk * wpc, w1 = min(nwtot, w0 + wpc);
  for (int win = w0; win < w1; ++win) {
    __syncthreads();                                    // the previous window's tiles have been consumed
    if (tid < NTOK) {
      int row, info;
      wa_token(g, win, tid, row, info);
      rows[tid] = row;
      infos[tid] = info;
    }
    __syncthreads();
    for (int idx = tid; idx < NTOK * 8; idx += NTHR) {
      const int n = idx >> 3, c4 = (idx & 7) * 4;
      const int row = rows[n];
      f32x4 q = {0.f, 0.f, 0.f, 0.f}, k = q, v = q, go = q;
      if (row >= 0) {
        const float* p = qkv + (size_t)row * C3 + h * 32 + c4;
        q = *reinterpret_cast<const f32x4*>(p) * scale;
        k = *reinterpret_cast<const f32x4*>(p + g.C);
        v = *reinterpret_cast<const f32x4*>(p + 2 * g.C);
        go = *reinterpret_cast<const f32x4*>(gout + (size_t)row * g.C + h * 32 + c4);
      }
      *reinterpret_cast<f32x4*>(Qs + n * WA_LD + c4) = q;
      *reinterpret_cast<f32x4*>(Ks + n * WA_LD + c4) = k;
      *reinterpret_cast<f32x4*>(Vs + n * WA_LD + c4) = v;
      *reinterpret_cast<f32x4*>(Gs + n * WA_LD + c4) = go;
    }
    __syncthreads();

    // ================= pass 1: this lane's QUERY i = n_own, keys j = 16 ct + 4 kq + r =================
    if (active) {
      const int ri = rows[n_own], ii = infos[n_own];
      const int bi = (ii & 0xffff) + bconst, regi = ii >> 16;
      float L = 0.f;
      if (ri >= 0) {
        const int b = ri / HW;
        L = lse[((size_t)b * g.heads + h) * HW + (ri - b * HW)];
      }
      const f32x4 qa = *reinterpret_cast<const f32x4*>(Qs + n_own * WA_LD + 8 * kq);
      const f32x4 qb = *reinterpret_cast<const f32x4*>(Qs + n_own * WA_LD + 8 * kq + 4);
      const f32x4 ga = *reinterpret_cast<const f32x4*>(Gs + n_own * WA_LD + 8 * kq);
      const f32x4 gb = *reinterpret_cast<const f32x4*>(Gs + n_own * WA_LD + 8 * kq + 4);
      f32x4 acc[NT], dp[NT];
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ct < nct) {
          acc[ct] = wa_dot8(Ks + (16 * ct + li) * WA_LD + 8 * kq, qa, qb, acc[ct]);       // S^T = K (scale Q)^T
          dp[ct] = wa_dot8(Vs + (16 * ct + li) * WA_LD + 8 * kq, ga, gb, dp[ct]);         // dP^T = V dO^T
        }
      }
      float dl = 0.f;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        if (ct < nct) {
          const wa_i32x4 ij = *reinterpret_cast<const wa_i32x4*>(infos + 16 * ct + 4 * kq);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = 16 * ct + 4 * kq + r;
            const float s = acc[ct][r] + tab[bi - (ij[r] & 0xffff)] + ((ij[r] >> 16) != regi ? -100.f : 0.f);
            const float p = (j < g.N && ri >= 0) ? __expf(s - L) : 0.f;
            acc[ct][r] = p;
            dl += p * dp[ct][r];
          }
        }
      }
      dl += __shfl_xor(dl, 16);
      dl += __shfl_xor(dl, 32);
      f32x4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = dq0;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        if (ct < nct) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float ds = acc[ct][r] * (dp[ct][r] - dl);
            tsum[ct][r] += ds;
            const float* kr = Ks + (16 * ct + 4 * kq + r) * WA_LD + li;                    // dQ^T = K^T dS^T
            dq0 = WA_MFMA(kr[0], ds, dq0);
            dq1 = WA_MFMA(kr[16], ds, dq1);
          }
        }
      }
      if (ri >= 0) {
        float* gp = gqkv + (size_t)ri * C3 + h * 32 + 4 * kq;
        *reinterpret_cast<f32x4*>(gp) = dq0 * scale;
        *reinterpret_cast<f32x4*>(gp + 16) = dq1 * scale;
      }
      if (kq == 0) {
        Ls[n_own] = L;
        Ds[n_own] = dl;
      }
    }
    __syncthreads();

    // ================= pass 2: this lane's KEY j = n_own, queries i = 16 ct + 4 kq + r =================
    if (active) {
      const int rj = rows[n_own], ijf = infos[n_own];
      const int bj = ijf & 0xffff, regj = ijf >> 16;
      const f32x4 ka = *reinterpret_cast<const f32x4*>(Ks + n_own * WA_LD + 8 * kq);
      const f32x4 kb = *reinterpret_cast<const f32x4*>(Ks + n_own * WA_LD + 8 * kq + 4);
      const f32x4 va = *reinterpret_cast<const f32x4*>(Vs + n_own * WA_LD + 8 * kq);
      const f32x4 vb = *reinterpret_cast<const f32x4*>(Vs + n_own * WA_LD + 8 * kq + 4);
      f32x4 dv0 = {0.f, 0.f, 0.f, 0.f}, dv1 = dv0, dk0 = dv0, dk1 = dv0;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        if (ct < nct) {
          const f32x4 z = {0.f, 0.f, 0.f, 0.f};
          const f32x4 acc = wa_dot8(Qs + (16 * ct + li) * WA_LD + 8 * kq, ka, kb, z);       // S = (scale Q) K^T
          const f32x4 dp = wa_dot8(Gs + (16 * ct + li) * WA_LD + 8 * kq, va, vb, z);        // dP = dO V^T
          const wa_i32x4 ii4 = *reinterpret_cast<const wa_i32x4*>(infos + 16 * ct + 4 * kq);
          const f32x4 L4 = *reinterpret_cast<const f32x4*>(Ls + 16 * ct + 4 * kq);
          const f32x4 D4 = *reinterpret_cast<const f32x4*>(Ds + 16 * ct + 4 * kq);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * ct + 4 * kq + r;
            const float s = acc[r] + tab[(ii4[r] & 0xffff) + bconst - bj] + ((ii4[r] >> 16) != regj ? -100.f : 0.f);
            const float p = (i < g.N && rj >= 0) ? __expf(s - L4[r]) : 0.f;
            const float ds = p * (dp[r] - D4[r]);
            const float* gr = Gs + i * WA_LD + li;                                         // dV^T = dO^T P
            const float* qr = Qs + i * WA_LD + li;                                         // dK^T = (scale Q)^T dS
            dv0 = WA_MFMA(gr[0], p, dv0);
            dv1 = WA_MFMA(gr[16], p, dv1);
            dk0 = WA_MFMA(qr[0], ds, dk0);
            dk1 = WA_MFMA(qr[16], ds, dk1);
          }
        }
      }
      if (rj >= 0) {
        float* gp = gqkv + (size_t)rj * C3 + g.C + h * 32 + 4 * kq;
        *reinterpret_cast<f32x4*>(gp) = dk0;
        *reinterpret_cast<f32x4*>(gp + 16) = dk1;
        *reinterpret_cast<f32x4*>(gp + g.C) = dv0;
        *reinterpret_cast<f32x4*>(gp + g.C + 16) = dv1;
      }
    }
  }

  // ---- grad_table partial of this (chunk, head): [N][N], dS summed over the chunk's windows ----
  if (active && n_own < g.N) {
    float* wp = wsp + ((size_t)chunk * g.heads + h) * g.N * g.N + (size_t)n_own * g.N;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      if (ct < nct) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * ct + 4 * kq + r;
          if (j < g.N) wp[j] = tsum[ct][r];
        }
      }
    }
  }
}

// grad_table[t][h] = sum over chunks and over the pairs (i, j) of a window whose coordinate difference is entry t, in a fixed order
__global__ __launch_bounds__(256) void cgg_window_attn_fold_kernel(const float* __restrict__ wsp, float* __restrict__ gtab, int ws,
                                                                   int heads, int nchunk) {
  __shared__ float red[256];
  const int t = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
  const int T1 = 2 * ws - 1, N = ws * ws;
  const int dy = t / T1 - (ws - 1), dx = t % T1 - (ws - 1);
  const int cy = ws - abs(dy), cx = ws - abs(dx), y0 = max(0, dy), x0 = max(0, dx);
  const int np = cy * cx, total = np * nchunk;
  float s = 0.f;
  for (int it = tid; it < total; it += 256) {
    const int c = it / np, p = it - c * np;
    const int py = p / cx, px = p - py * cx;
    const int yi = y0 + py, xi = x0 + px;
    const int i = yi * ws + xi, j = (yi - dy) * ws + (xi - dx);
    s += wsp[(((size_t)c * heads + h) * N + i) * N + j];
  }
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) gtab[(size_t)t * heads + h] = red[0];
}

static int wa_check_shape(const char* who, int B, int Hp, int Wp, int C, int heads, int ws, int shift) {
  CGG_REQUIRE(B > 0 && Hp > 0 && Wp > 0 && C > 0 && heads > 0 && ws > 0, CGG_EINVAL, "%s: bad sizes", who);
  CGG_REQUIRE(C == heads * 32, CGG_EUNSUPPORTED, "%s: C=%d with %d heads (only head dim 32 is built)", who, C, heads);
  CGG_REQUIRE(ws * ws <= 144, CGG_EUNSUPPORTED, "%s: window %d x %d > 144 tokens", who, ws, ws);
  CGG_REQUIRE(Hp % ws == 0 && Wp % ws == 0, CGG_EUNSUPPORTED, "%s: map %d x %d is not a multiple of the window %d (pad first)", who,
              Hp, Wp, ws);
  CGG_REQUIRE(shift >= 0 && shift < ws, CGG_EUNSUPPORTED, "%s: shift %d outside [0, %d)", who, shift, ws);
  CGG_REQUIRE((int64_t)B * Hp * Wp < (int64_t)1 << 31, CGG_EUNSUPPORTED, "%s: more than 2^31 tokens", who);
  return CGG_OK;
}

static WaShape wa_shape(int Hp, int Wp, int C, int heads, int ws, int shift) {
  WaShape g;
  g.Hp = Hp, g.Wp = Wp, g.C = C, g.heads = heads, g.ws = ws, g.shift = shift;
  g.N = ws * ws, g.nwx = Wp / ws, g.nwin = (Hp / ws) * (Wp / ws);
  return g;
}

// windows per workgroup of the backward: ~2 workgroups per CU over (chunk, head)
static void wa_bwd_plan(int nwtot, int heads, int* wpc, int* nchunk) {
  int want = (512 + heads - 1) / heads;
  if (want > nwtot) want = nwtot;
  if (want < 1) want = 1;
  *wpc = (nwtot + want - 1) / want;
  *nchunk = (nwtot + *wpc - 1) / *wpc;
}

extern "C" int cgg_window_attn_forward(const float* qkv, const float* table, float* out, float* lse, int B, int Hp, int Wp, int C,
                                       int heads, int ws, int shift, float scale, cgg_stream_t stream) {
  CGG_REQUIRE(qkv && table && out && lse, CGG_EINVAL, "cgg_window_attn_forward: null pointer");
  const int rc = wa_check_shape("cgg_window_attn_forward", B, Hp, Wp, C, heads, ws, shift);
  if (rc != CGG_OK) return rc;
  CGG_REQUIRE(cgg_aligned16(qkv) && cgg_aligned16(out), CGG_EALIGN, "cgg_window_attn_forward: qkv and out must be 16-B aligned");
  const WaShape g = wa_shape(Hp, Wp, C, heads, ws, shift);
  const dim3 grid((unsigned)(B * g.nwin), (unsigned)heads);
  hipStream_t s = (hipStream_t)stream;
  if (g.N <= 64) {
    const size_t lds = (size_t)(2 * 64 * WA_LD + WA_TAB + 2 * 64) * sizeof(float);
    hipLaunchKernelGGL(cgg_window_attn_fwd_kernel<4>, grid, dim3(256), lds, s, qkv, table, out, lse, g, scale);
  } else {
    const size_t lds = (size_t)(2 * 144 * WA_LD + WA_TAB + 2 * 144) * sizeof(float);
    hipLaunchKernelGGL(cgg_window_attn_fwd_kernel<9>, grid, dim3(576), lds, s, qkv, table, out, lse, g, scale);
  }
  CGG_CHECK_LAUNCH("cgg_window_attn_forward");
  return CGG_OK;
}

extern "C" int64_t cgg_window_attn_backward_workspace_bytes(int B, int Hp, int Wp, int heads, int ws) {
  if (B <= 0 || Hp <= 0 || Wp <= 0 || heads <= 0 || ws <= 0 || Hp % ws != 0 || Wp % ws != 0) return 0;
  int wpc, nchunk;
  wa_bwd_plan(B * (Hp / ws) * (Wp / ws), heads, &wpc, &nchunk);
  return (int64_t)nchunk * heads * ws * ws * ws * ws * (int64_t)sizeof(float);
}

extern "C" int cgg_window_attn_backward(const float* qkv, const float* table, const float* lse, const float* grad_out, float* grad_qkv,
                                        float* grad_table, void* ws_buf, int B, int Hp, int Wp, int C, int heads, int ws, int shift,
                                        float scale, cgg_stream_t stream) {
  CGG_REQUIRE(qkv && table && lse && grad_out && grad_qkv && grad_table && ws_buf, CGG_EINVAL,
              "cgg_window_attn_backward: null pointer");
  const int rc = wa_check_shape("cgg_window_attn_backward", B, Hp, Wp, C, heads, ws, shift);
  if (rc != CGG_OK) return rc;
  CGG_REQUIRE(cgg_aligned16(qkv) && cgg_aligned16(grad_out) && cgg_aligned16(grad_qkv) && cgg_aligned16(ws_buf), CGG_EALIGN,
              "cgg_window_attn_backward: qkv, grad_out, grad_qkv and the workspace must be 16-B aligned");
  const WaShape g = wa_shape(Hp, Wp, C, heads, ws, shift);
  const int nwtot = B * g.nwin;
  int wpc, nchunk;
  wa_bwd_plan(nwtot, heads, &wpc, &nchunk);
  const dim3 grid((unsigned)nchunk, (unsigned)heads);
  hipStream_t s = (hipStream_t)stream;
  if (g.N <= 64) {
    const size_t lds = (size_t)(4 * 64 * WA_LD + WA_TAB + 4 * 64) * sizeof(float);
    hipLaunchKernelGGL(cgg_window_attn_bwd_kernel<4>, grid, dim3(256), lds, s, qkv, table, lse, grad_out, grad_qkv, (float*)ws_buf, g,
                       scale, wpc, nwtot);
  } else {
    const size_t lds = (size_t)(4 * 144 * WA_LD + WA_TAB + 4 * 144) * sizeof(float);      // 87 KB: above the 64 KB default limit
    CGG_RAISE_LDS(cgg_window_attn_bwd_kernel<9>, lds, "cgg_window_attn_backward(main)");
    hipLaunchKernelGGL(cgg_window_attn_bwd_kernel<9>, grid, dim3(576), lds, s, qkv, table, lse, grad_out, grad_qkv, (float*)ws_buf, g,
                       scale, wpc, nwtot);
  }
  CGG_CHECK_LAUNCH("cgg_window_attn_backward(main)");
  const int T1 = 2 * ws - 1;
  hipLaunchKernelGGL(cgg_window_attn_fold_kernel, dim3((unsigned)(T1 * T1), (unsigned)heads), dim3(256), 0, s, (const float*)ws_buf,
                     grad_table, ws, heads, nchunk);
  CGG_CHECK_LAUNCH("cgg_window_attn_backward(fold)");
  return CGG_OK;
}
