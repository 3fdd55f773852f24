// Bahdanau ("mlp") attention, forward and backward, for gfx950 (reference: onmt/modules/GlobalAttention.py:70-78 parameters,
// :114-127 score, :171-184 mask / softmax / context).
//   score[t][s] = v . tanh(W_q r_t + b_q + W_c Hs_s)     (wq = W_q r and uh = W_c Hs arrive from two GEMMs)
//   a = softmax over s < len ; c[t] = sum_s a[t][s] Hs[s]  -> columns [0,H) of the [c ; r] concat buffer
// The tanh sits inside the reduction over h, so the score is no matrix product: it is VALU + transcendental work, H tanh per (t, s) pair.
// Only c = A Hs (forward), dP = dC Hs^T and dHs = P^T dC (backward) are products and go through the matrix pipe.
//
// Forward, bf16, S <= 64 (attn_mlp_fwd_lds): grid (sentence, 16 - 64 queries); ONE LDS region serves two phases --
//   1. uh_b [S x H] staged; (query, four positions) units are dealt round-robin to the four waves (a single decode query keeps all of them busy), lanes
//      lie across h in 16-byte vectors, four wave reductions in flight; scores, then probabilities, stay in LDS;
//   2. the region is restaged with Hs_b and the contexts are 32 x 32 MFMA tiles P (bf16) x Hs, Hs read K-strided from the same image.
// Backward, bf16, S, T' <= 64 (attn_mlp_bwd_kernel<bf16, true>): grid (sentence, 256 columns of H); every workgroup recomputes
//   dP = dC Hs^T (one 32 x 32 MFMA tile per wave, fragments straight from global memory) and dS = P (dP - sum P dP); then thread = column h:
//   eight positions' uh and duh sums at a time in registers over the loop over t, dwq[t][h] in an f32 LDS tile that only its owner
//   touches, dv[h] in a register (one partial row per sentence, folded by the caller with vmmt_colsum: no floating-point atomics); dHs = P^T dC through the matrix pipe.
// Backward, S or T' > 64 (attn_mlp_bwd_long_*, S <= 256, any T'): the work cut along T' into four launches, see below.
// b_q is added once per query in f32, next to the query's registers: a staged bf16 image of uh + b_q would round the sum a second time.
// Precondition shared with vmmt_attn_fwd: lens[b] >= 1 (an empty sentence gets zero probabilities and a zero context).
// Everything else (fp32 parity mode, S > 64 in the forward, unaligned rows): plain kernels with the same arithmetic.
#include "common.hpp"
#include "vmmt.h"

namespace vmmt {
namespace {

constexpr int AM_MAXJ = 16;    // H <= 1024
constexpr int AM_LK = 4;       // S <= 256 (forward, one wave per query)
constexpr int AM_MAXS = 64;    // per-sentence kernels: S <= 64, and 64 queries per workgroup
constexpr int AM_SC = 65;      // pitch of the f32 [64][64] score / dS tables
constexpr int AM_PB = 72;      // pitch of the bf16 [64][64] probability image
constexpr int AM_HC = 256;     // backward: columns of H per workgroup (one per thread)

// the ONE tanh of this file (common.hpp's cell_tanh_: v_exp_f32 + v_rcp_f32): the backward recomputes exactly what the forward used
__device__ __forceinline__ float mlp_tanh(float x) { return cell_tanh_(x); }

typedef short am16x4 __attribute__((ext_vector_type(4)));
typedef short am16x8 __attribute__((ext_vector_type(8)));
// MFMA 32x32x16 operand fragments: K-contiguous image [row][k] / K-strided image [k][row] (ds_read_b64_tr_b16) / global rows
__device__ __forceinline__ bf16x8 fragKC(const bf16_t* img, int stride, int row0, int kbase, int lane) {
  return *reinterpret_cast<const bf16x8*>(img + (row0 + (lane & 31)) * stride + kbase + 8 * (lane >> 5));
}
__device__ __forceinline__ bf16x8 fragKS(const bf16_t* img, int stride, int row0, int kbase, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const bf16_t* a0 = img + (kbase + 8 * (g >> 1) + q) * stride + row0 + 16 * (g & 1) + 4 * p;
  typedef __attribute__((address_space(3))) am16x4 lds_v;
  am16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v*)(a0));
  am16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v*)(a0 + 4 * stride));
  am16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ bf16x8 fragG(const bf16_t* base, long rstride, int row0, int nrows, int kbase, int lane) {
  const int r = row0 + (lane & 31);
  u32x4 v = {0u, 0u, 0u, 0u};
  if (r < nrows) v = *reinterpret_cast<const u32x4*>(base + (long)r * rstride + kbase + 8 * (lane >> 5));
  return __builtin_bit_cast(bf16x8, v);
}
// stage `rows` rows of `cols` elements (row r from src + r*rstride; rows >= nrows are zero-filled) into a [rows][pitch] image
__device__ __forceinline__ void stage_rows(bf16_t* img, int pitch, const bf16_t* src, long rstride, int nrows, int rows, int cols) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int r = wave; r < rows; r += 4) {
    const bf16_t* g = src + (long)r * rstride;
    for (int c = lane * 8; c < cols; c += 512) {
      u32x4 v = zero;
      if (r < nrows) v = *reinterpret_cast<const u32x4*>(g + c);
      *reinterpret_cast<u32x4*>(img + r * pitch + c) = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// forward, bf16, S <= 64, H % 32 == 0, 16-byte rows
__global__ void __launch_bounds__(256) attn_mlp_fwd_lds(const bf16_t* __restrict__ wq, long ldwq, const float* __restrict__ bq,
                                                        const bf16_t* __restrict__ uh, long lduh, const float* __restrict__ v,
                                                        const bf16_t* __restrict__ ctx, long ldc, const long long* __restrict__ lens,
                                                        bf16_t* __restrict__ cat, long ldcat, float* __restrict__ probs, int Tp, int B,
                                                        int S, int H, int tq) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int P = H + 8, rows32 = (S + 31) & ~31;
  bf16_t* img = reinterpret_cast<bf16_t*>(smem_raw);                       // [rows32][P]: uh_b, then Hs_b
  float* sc = reinterpret_cast<float*>(img + rows32 * P);                  // [64][AM_SC]
  bf16_t* Pb = reinterpret_cast<bf16_t*>(sc + AM_MAXS * AM_SC);            // [64][AM_PB]
  const int b = blockIdx.x, t0 = blockIdx.y * tq, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nT = min(tq, Tp - t0);
  int len = (int)lens[b];
  len = len < S ? len : S;
  stage_rows(img, P, uh + (long)b * lduh, (long)B * lduh, S, rows32, H);
  // this lane's hidden units: h = 8 lane + 512 j + e
  float vv[AM_MAXJ], bb[AM_MAXJ], qv[AM_MAXJ];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int h = 8 * lane + 512 * j + e;
      vv[8 * j + e] = h < H ? v[h] : 0.f;
      bb[8 * j + e] = h < H ? bq[h] : 0.f;
      qv[8 * j + e] = 0.f;
    }
  __syncthreads();
  // phase 1: scores; a unit of work is (query, four positions): four independent reductions in flight per wave
  int tcur = -1;
  const int nblk = (len + 3) >> 2;
  for (int i = wave; i < nT * nblk; i += 4) {
    const int t = i / nblk, s0 = (i - t * nblk) * 4;
    if (t != tcur) {
      const bf16_t* qr = wq + ((long)(t0 + t) * B + b) * ldwq;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = 8 * lane + 512 * j;
        if (c < H) {
          const u32x4 raw = *reinterpret_cast<const u32x4*>(qr + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            qv[8 * j + 2 * e] = __uint_as_float(raw[e] << 16) + bb[8 * j + 2 * e];
            qv[8 * j + 2 * e + 1] = __uint_as_float(raw[e] & 0xffff0000u) + bb[8 * j + 2 * e + 1];
          }
        }
      }
      tcur = t;
    }
    float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = 8 * lane + 512 * j;
      if (c < H) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const u32x4 raw = *reinterpret_cast<const u32x4*>(img + min(s0 + u, len - 1) * P + c);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            part[u] += vv[8 * j + 2 * e] * mlp_tanh(qv[8 * j + 2 * e] + __uint_as_float(raw[e] << 16));
            part[u] += vv[8 * j + 2 * e + 1] * mlp_tanh(qv[8 * j + 2 * e + 1] + __uint_as_float(raw[e] & 0xffff0000u));
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) part[u] = wave_sum(part[u]);
    const float mine = lane == 0 ? part[0] : lane == 1 ? part[1] : lane == 2 ? part[2] : part[3];
    if (lane < 4 && s0 + lane < len) sc[t * AM_SC + s0 + lane] = mine;
  }
  __syncthreads();                                   // scores complete; nobody reads uh_b any more
  stage_rows(img, P, ctx + (long)b * ldc, (long)B * ldc, S, rows32, H);
  for (int t = wave; t < AM_MAXS; t += 4) {          // softmax, one query per wave pass (rows >= nT: zeros for the MFMA)
    const bool on = t < nT && lane < len;
    const float x = on ? sc[t * AM_SC + lane] : -INFINITY;
    const float m = wave_max(x);
    const float e = on ? __expf(x - m) : 0.f;
    const float sum = wave_sum(e);
    const float p = (t < nT && sum > 0.f) ? e / sum : 0.f;        // (an empty sentence, len = 0: zeros, not 0 / 0)
    if (t < nT && lane < S) probs[((long)(t0 + t) * B + b) * S + lane] = p;
    Pb[t * AM_PB + lane] = f2bf(p);
  }
  __syncthreads();
  // phase 2: contexts, 32 x 32 tiles (t-tile, 32 hidden units) dealt round-robin to the waves
  const int rows_t = (nT + 15) & ~15, nht = H / 32, nks = ((S + 15) & ~15) / 16;
  for (int idx = wave; idx < (rows_t + 31) / 32 * nht; idx += 4) {
    const int tt = (idx / nht) * 32, h0 = (idx % nht) * 32;
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    for (int ks = 0; ks < nks; ++ks)
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fragKC(Pb, AM_PB, tt, ks * 16, lane), fragKS(img, P, h0, ks * 16, lane), c, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = tt + acc_row(r, lane);
      if (t < nT) cat[((long)(t0 + t) * B + b) * ldcat + h0 + (lane & 31)] = f2bf(c[r]);
    }
  }
}

// forward, any dtype, S <= 256: one wave per (sentence, query); lanes hold the positions s = lane + 64 k and the hidden units
// h = lane + 64 j; uh and Hs straight from global memory / L2
template <class T>
__global__ void __launch_bounds__(256) attn_mlp_fwd_wave(const T* __restrict__ wq, long ldwq, const float* __restrict__ bq,
                                                         const T* __restrict__ uh, long lduh, const float* __restrict__ v,
                                                         const T* __restrict__ ctx, long ldc, const long long* __restrict__ lens,
                                                         T* __restrict__ cat, long ldcat, float* __restrict__ probs, int Tp, int B, int S,
                                                         int H) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + wave;             // row = t * B + b
  if (row >= (long)Tp * B) return;
  const int b = (int)(row % B);
  int len = (int)lens[b];
  len = len < S ? len : S;
  const T* qr = wq + row * ldwq;
  float qv[AM_MAXJ], vv[AM_MAXJ];
#pragma unroll
  for (int j = 0; j < AM_MAXJ; ++j) {
    const int h = lane + 64 * j;
    qv[j] = h < H ? to_f<T>(qr[h]) + bq[h] : 0.f;
    vv[j] = h < H ? v[h] : 0.f;
  }
  float my[AM_LK];
#pragma unroll
  for (int k = 0; k < AM_LK; ++k) my[k] = -INFINITY;
  for (int s = 0; s < len; ++s) {
    const T* ur = uh + ((long)s * B + b) * lduh;
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < AM_MAXJ; ++j)
      if (lane + 64 * j < H) part += vv[j] * mlp_tanh(qv[j] + to_f<T>(ur[lane + 64 * j]));
    part = wave_sum(part);
#pragma unroll
    for (int k = 0; k < AM_LK; ++k)
      if ((s >> 6) == k && lane == (s & 63)) my[k] = part;
  }
  float m = my[0];
#pragma unroll
  for (int k = 1; k < AM_LK; ++k) m = fmaxf(m, my[k]);
  m = wave_max(m);
  float pk[AM_LK], sum = 0.f;
#pragma unroll
  for (int k = 0; k < AM_LK; ++k) { pk[k] = lane + 64 * k < len ? __expf(my[k] - m) : 0.f; sum += pk[k]; }
  sum = wave_sum(sum);
#pragma unroll
  for (int k = 0; k < AM_LK; ++k) {
    pk[k] = sum > 0.f ? pk[k] / sum : 0.f;                      // (an empty sentence, len = 0: zeros, not 0 / 0)
    if (lane + 64 * k < S) probs[row * S + lane + 64 * k] = pk[k];
  }
  float acc[AM_MAXJ];
#pragma unroll
  for (int j = 0; j < AM_MAXJ; ++j) acc[j] = 0.f;
  for (int s = 0; s < len; ++s) {
    float ps = 0.f;
#pragma unroll
    for (int k = 0; k < AM_LK; ++k) { const float x = __shfl(pk[k], s & 63, 64); ps = (s >> 6) == k ? x : ps; }
    const T* hr = ctx + ((long)s * B + b) * ldc;
#pragma unroll
    for (int j = 0; j < AM_MAXJ; ++j)
      if (lane + 64 * j < H) acc[j] += ps * to_f<T>(hr[lane + 64 * j]);
  }
  T* cr = cat + row * ldcat;
#pragma unroll
  for (int j = 0; j < AM_MAXJ; ++j)
    if (lane + 64 * j < H) cr[lane + 64 * j] = from_f<T>(acc[j]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward, S, T' <= 64: workgroup (sentence b, columns [c0, c0 + 256) of H).  FAST: bf16, H % 32 == 0, 16-byte rows.
template <class T, bool FAST>
__global__ void __launch_bounds__(256) attn_mlp_bwd_kernel(const T* __restrict__ dcat, long lddc, const float* __restrict__ probs,
                                                           const T* __restrict__ wq, long ldwq, const float* __restrict__ bq,
                                                           const T* __restrict__ uh, long lduh, const float* __restrict__ v,
                                                           const T* __restrict__ ctx, long ldc, const long long* __restrict__ lens,
                                                           T* __restrict__ dwq, long lddwq, T* __restrict__ duh, long ldduh,
                                                           T* __restrict__ dctx, long lddx, float* __restrict__ dv_part, int Tp, int B,
                                                           int S, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* dsb = reinterpret_cast<float*>(smem_raw);                         // [64][AM_SC]: dP, then dS
  float* acc_t = dsb + AM_MAXS * AM_SC;                                    // [T'][AM_HC] f32: dwq of this thread's column
  float* pb = acc_t + Tp * AM_HC;                                          // !FAST: [64][AM_SC] probabilities
  bf16_t* Pb = reinterpret_cast<bf16_t*>(acc_t + Tp * AM_HC);              // FAST: [64][AM_PB] probabilities (bf16, MFMA operand)
  bf16_t* wqt = Pb + AM_MAXS * AM_PB;                                      // FAST: [T'][AM_HC] wq columns, later dC chunk [rows_t][PC]
  const int b = blockIdx.x, c0 = blockIdx.y * AM_HC, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nc = min(AM_HC, H - c0), h = c0 + tid;
  const bool mine = tid < nc;
  int len = (int)lens[b];
  len = len < S ? len : S;
  for (int t = 0; t < Tp; ++t) {
    acc_t[t * AM_HC + tid] = 0.f;
    if constexpr (FAST)
      if (mine) wqt[t * AM_HC + tid] = (bf16_t)wq[((long)t * B + b) * ldwq + h];
  }
  // ---- dP = dC Hs^T, dS = P (dP - sum_s P dP)
  if constexpr (FAST) {
    const int tt = wave >> 1, st = wave & 1;
    if (tt * 32 < Tp && st * 32 < S) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const bf16_t* db = reinterpret_cast<const bf16_t*>(dcat) + (long)b * lddc;
      const bf16_t* cb = reinterpret_cast<const bf16_t*>(ctx) + (long)b * ldc;
      for (int k0 = 0; k0 < H; k0 += 64) {
        bf16x8 fa[4], fb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = k0 + 16 * j < H;
          fa[j] = fragG(db, (long)B * lddc, tt * 32, in ? Tp : 0, in ? k0 + 16 * j : 0, lane);
          fb[j] = fragG(cb, (long)B * ldc, st * 32, in ? S : 0, in ? k0 + 16 * j : 0, lane);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k0 + 16 * j < H) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[j], fb[j], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) dsb[(tt * 32 + acc_row(r, lane)) * AM_SC + st * 32 + (lane & 31)] = acc[r];
    }
    __syncthreads();
    for (int t = wave; t < AM_MAXS; t += 4) {        // (rows >= T': zeros for the MFMA)
      const bool on = t < Tp && lane < len;
      const float p = on ? probs[((long)t * B + b) * S + lane] : 0.f;
      const float dp = on ? dsb[t * AM_SC + lane] : 0.f;
      const float dot = wave_sum(p * dp);
      dsb[t * AM_SC + lane] = p * (dp - dot);
      Pb[t * AM_PB + lane] = f2bf(p);
    }
  } else {
    for (int t = wave; t < Tp; t += 4) {
      const T* dcr = dcat + ((long)t * B + b) * lddc;
      float dp = 0.f;
      for (int s = 0; s < len; ++s) {
        const T* hr = ctx + ((long)s * B + b) * ldc;
        float part = 0.f;
        for (int k = lane; k < H; k += 64) part += to_f<T>(dcr[k]) * to_f<T>(hr[k]);
        part = wave_sum(part);
        if (lane == s) dp = part;
      }
      const float p = lane < len ? probs[((long)t * B + b) * S + lane] : 0.f;
      const float dot = wave_sum(p * dp);
      dsb[t * AM_SC + lane] = p * (dp - dot);
      pb[t * AM_SC + lane] = p;
    }
  }
  __syncthreads();
  // ---- the tanh part: this thread's column h.  Eight source positions at a time: their uh and their duh sums live in registers over
  // the loop over t, and dwq[t][h] passes through the LDS tile once per eight tanh
  if (mine) {
    const float vh = v[h], bh = bq[h];
    float dv = 0.f;
    for (int s0 = 0; s0 < len; s0 += 8) {
      float u[8], du[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        u[k] = to_f<T>(uh[((long)min(s0 + k, len - 1) * B + b) * lduh + h]);      // tail: a valid row again, its terms are dropped below
        du[k] = 0.f;
      }
      for (int t = 0; t < Tp; ++t) {
        float a;
        if constexpr (FAST) a = bf2f(wqt[t * AM_HC + tid]) + bh;
        else a = to_f<T>(wq[((long)t * B + b) * ldwq + h]) + bh;
        float acc = acc_t[t * AM_HC + tid];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const bool on = s0 + k < len;
          const float d = dsb[t * AM_SC + s0 + k];          // s0 is a multiple of 8 below len <= 64: s0 + k <= 63, inside the row
          const float th = mlp_tanh(a + u[k]);
          const float g = on ? d * vh * (1.f - th * th) : 0.f;
          acc += g;
          du[k] += g;
          dv += on ? d * th : 0.f;
        }
        acc_t[t * AM_HC + tid] = acc;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (s0 + k < len) duh[((long)(s0 + k) * B + b) * ldduh + h] = from_f<T>(du[k]);
    }
    for (int s = len; s < S; ++s) duh[((long)s * B + b) * ldduh + h] = from_f<T>(0.f);                   // zero at pads
    for (int t = 0; t < Tp; ++t) dwq[((long)t * B + b) * lddwq + h] = from_f<T>(acc_t[t * AM_HC + tid]);
    dv_part[(long)b * H + h] = dv;
  }
  // ---- dHs[s][h] = sum_t P[t][s] dC[t][h] (the direct path only), zero at pads
  if constexpr (FAST) {
    const int PC = AM_HC + 8, rows_t = (Tp + 15) & ~15, rows_s = (S + 15) & ~15;
    __syncthreads();                                 // everybody is done with the wq columns
    bf16_t* dCs = wqt;                               // [rows_t][PC]
    stage_rows(dCs, PC, reinterpret_cast<const bf16_t*>(dcat) + (long)b * lddc + c0, (long)B * lddc, Tp, rows_t, nc);
    __syncthreads();
    const int nhc = nc / 32, nkt = rows_t / 16;
    bf16_t* out = reinterpret_cast<bf16_t*>(dctx);
    for (int idx = wave; idx < (rows_s + 31) / 32 * nhc; idx += 4) {
      const int s0 = (idx / nhc) * 32, h0 = (idx % nhc) * 32;
      f32x16 c;
#pragma unroll
      for (int r = 0; r < 16; ++r) c[r] = 0.f;
      for (int ks = 0; ks < nkt; ++ks)
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fragKS(Pb, AM_PB, s0, ks * 16, lane), fragKS(dCs, PC, h0, ks * 16, lane), c, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int srow = s0 + acc_row(r, lane);
        if (srow < S) out[((long)srow * B + b) * lddx + c0 + h0 + (lane & 31)] = f2bf(srow < len ? c[r] : 0.f);
      }
    }
  } else if (mine) {
    for (int s0 = 0; s0 < S; s0 += 8) {
      float dx[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) dx[k] = 0.f;
      for (int t = 0; t < Tp; ++t) {
        const float x = to_f<T>(dcat[((long)t * B + b) * lddc + h]);
#pragma unroll
        for (int k = 0; k < 8; ++k) dx[k] += s0 + k < len ? pb[t * AM_SC + s0 + k] * x : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (s0 + k < S) dctx[((long)(s0 + k) * B + b) * lddx + h] = from_f<T>(dx[k]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward beyond the per-sentence kernel: S <= 256, any T' (vmmt_attn_mlp_bwd_long).  The whole-sentence LDS tiles of the kernel above
// do not survive T' = 256 or S = 256, so the work is cut along T' and handed on through caller-owned f32 scratch:
//   1. attn_mlp_bwd_long_ds   (sentence, 32 queries): dP = dC Hs^T for ALL of S inside the workgroup (the row sum of the softmax backward
//      stays local), dS = P (dP - sum P dP) written f32 [T' B][S], the layout of probs;
//   2. attn_mlp_bwd_long_tanh (sentence, 256 columns of H, chunk of AM_LTC queries): thread = column, the loop of the short kernel over
//      the chunk's dS rows staged in LDS; dwq rows belong to exactly one chunk and are final; duh and dv are one f32 partial per chunk;
//   3. attn_mlp_bwd_long_dhs  (sentence, 256 columns of H, 64 positions): dHs = P^T dC over all of T', 64 queries staged at a time;
//   4. attn_mlp_bwd_long_fold: duh = the chunks' partials added in chunk order (skipped when T' fits one chunk: the tanh kernel then
//      writes duh itself).  dv's partial rows are folded by the caller with vmmt_colsum, as for the short kernel.
// The chunk is a grid dimension, not a loop: long sentences come in small batches, and B * ceil(H / 256) workgroups leave most of the
// chip idle.  Fixed order everywhere, no floating-point atomics: two calls return the same bits.
constexpr int AM_LQ = 32;      // queries per workgroup of the dS kernel (one MFMA tile row)
constexpr int AM_LDP = 257;    // pitch of its f32 [32][256] dP table
constexpr int AM_LTC = 32;     // queries per chunk of the tanh kernel: 80 KB of LDS at S = 256 in bf16, two workgroups per compute unit

template <class T, bool FAST>
__global__ void __launch_bounds__(256) attn_mlp_bwd_long_ds(const T* __restrict__ dcat, long lddc, const float* __restrict__ probs,
                                                            const T* __restrict__ ctx, long ldc, const long long* __restrict__ lens,
                                                            float* __restrict__ dS, int Tp, int B, int S, int H) {
  __shared__ float dpt[FAST ? AM_LQ * AM_LDP : 1];
  const int b = blockIdx.x, t0 = blockIdx.y * AM_LQ, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int len = (int)lens[b];
  len = len < S ? len : S;
  if constexpr (FAST) {
    // position tiles `wave` and `wave + 4`: the dC fragments of a k-step are loaded once and serve both
    const int sa = wave * 32, sb = sa + 128;
    const bool two = sb < len;
    if (sa < len) {
      f32x16 acc0, acc1;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
      const bf16_t* db = reinterpret_cast<const bf16_t*>(dcat) + (long)b * lddc;
      const bf16_t* cb = reinterpret_cast<const bf16_t*>(ctx) + (long)b * ldc;
      for (int k0 = 0; k0 < H; k0 += 64) {
        bf16x8 fa[4], fb0[4], fb1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = k0 + 16 * j < H;
          const int kb = in ? k0 + 16 * j : 0;
          fa[j] = fragG(db, (long)B * lddc, t0, in ? Tp : 0, kb, lane);
          fb0[j] = fragG(cb, (long)B * ldc, sa, in ? S : 0, kb, lane);
          fb1[j] = fragG(cb, (long)B * ldc, sb, in && two ? S : 0, kb, lane);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k0 + 16 * j < H) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[j], fb0[j], acc0, 0, 0, 0);
            if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[j], fb1[j], acc1, 0, 0, 0);
          }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        dpt[acc_row(r, lane) * AM_LDP + sa + (lane & 31)] = acc0[r];
        if (two) dpt[acc_row(r, lane) * AM_LDP + sb + (lane & 31)] = acc1[r];
      }
    }
    __syncthreads();
  }
  // one query per wave pass; lanes hold the positions s = lane + 64 k
  for (int tt = wave; tt < AM_LQ && t0 + tt < Tp; tt += 4) {
    const long row = (long)(t0 + tt) * B + b;
    float dp[AM_LK], p[AM_LK];
#pragma unroll
    for (int k = 0; k < AM_LK; ++k) dp[k] = 0.f;
    if constexpr (FAST) {
#pragma unroll
      for (int k = 0; k < AM_LK; ++k)
        if (lane + 64 * k < len) dp[k] = dpt[tt * AM_LDP + lane + 64 * k];      // (tiles at or beyond len were not computed)
    } else {
      const T* dcr = dcat + row * lddc;
      float dc[AM_MAXJ];
#pragma unroll
      for (int j = 0; j < AM_MAXJ; ++j) dc[j] = lane + 64 * j < H ? to_f<T>(dcr[lane + 64 * j]) : 0.f;
      for (int s = 0; s < len; ++s) {
        const T* hr = ctx + ((long)s * B + b) * ldc;
        float part = 0.f;
#pragma unroll
        for (int j = 0; j < AM_MAXJ; ++j)
          if (lane + 64 * j < H) part += dc[j] * to_f<T>(hr[lane + 64 * j]);
        part = wave_sum(part);
#pragma unroll
        for (int k = 0; k < AM_LK; ++k)
          if ((s >> 6) == k && lane == (s & 63)) dp[k] = part;
      }
    }
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < AM_LK; ++k) {
      p[k] = lane + 64 * k < len ? probs[row * S + lane + 64 * k] : 0.f;
      dot += p[k] * dp[k];
    }
    dot = wave_sum(dot);
#pragma unroll
    for (int k = 0; k < AM_LK; ++k)
      if (lane + 64 * k < S) dS[row * S + lane + 64 * k] = p[k] * (dp[k] - dot);          // zero at pads
  }
}

// the tanh part for one chunk of queries [t0, t0 + AM_LTC): the short kernel's loop (eight positions' uh and duh sums in registers over the
// loop over t, dwq[t][h] in an owner-only f32 LDS tile), over all of S.  bf16: the chunk's wq columns are staged next to the tile.
template <class T>
__global__ void __launch_bounds__(256) attn_mlp_bwd_long_tanh(const float* __restrict__ dS, const T* __restrict__ wq, long ldwq,
                                                              const float* __restrict__ bq, const T* __restrict__ uh, long lduh,
                                                              const float* __restrict__ v, const long long* __restrict__ lens,
                                                              T* __restrict__ dwq, long lddwq, T* __restrict__ duh, long ldduh,
                                                              float* __restrict__ duh_part, float* __restrict__ dv_part, int Tp, int B,
                                                              int S, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr bool STAGE = sizeof(T) == 2;
  const int pitch = (S + 7) & ~7;                                          // a block of eight positions never leaves its row
  float* dsb = reinterpret_cast<float*>(smem_raw);                         // [AM_LTC][pitch]: the chunk's dS rows
  float* acc_t = dsb + AM_LTC * pitch;                                     // [AM_LTC][AM_HC] f32: dwq of this thread's column
  bf16_t* wqt = reinterpret_cast<bf16_t*>(acc_t + AM_LTC * AM_HC);         // STAGE: [AM_LTC][AM_HC] wq columns
  const int b = blockIdx.x, c0 = blockIdx.y * AM_HC, ch = blockIdx.z, nch = gridDim.z, t0 = ch * AM_LTC, tid = threadIdx.x;
  const int nT = min(AM_LTC, Tp - t0), nc = min(AM_HC, H - c0), h = c0 + tid;
  const bool mine = tid < nc;
  int len = (int)lens[b];
  len = len < S ? len : S;
  for (int t = 0; t < nT; ++t) {
    acc_t[t * AM_HC + tid] = 0.f;
    if constexpr (STAGE)
      if (mine) wqt[t * AM_HC + tid] = (bf16_t)wq[((long)(t0 + t) * B + b) * ldwq + h];
  }
  for (int i = tid; i < AM_LTC * pitch; i += 256) {
    const int t = i / pitch, s = i - t * pitch;
    dsb[i] = (t < nT && s < S) ? dS[((long)(t0 + t) * B + b) * S + s] : 0.f;
  }
  __syncthreads();
  if (!mine) return;
  const float vh = v[h], bh = bq[h];
  float dv = 0.f;
  for (int s0 = 0; s0 < len; s0 += 8) {
    float u[8], du[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      u[k] = to_f<T>(uh[((long)min(s0 + k, len - 1) * B + b) * lduh + h]);      // tail: a valid row again, its terms are dropped below
      du[k] = 0.f;
    }
    for (int t = 0; t < nT; ++t) {
      float a;
      if constexpr (STAGE) a = bf2f(wqt[t * AM_HC + tid]) + bh;
      else a = to_f<T>(wq[((long)(t0 + t) * B + b) * ldwq + h]) + bh;
      const f32x4 d0 = *reinterpret_cast<const f32x4*>(dsb + t * pitch + s0), d1 = *reinterpret_cast<const f32x4*>(dsb + t * pitch + s0 + 4);
      float acc = acc_t[t * AM_HC + tid];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool on = s0 + k < len;
        const float d = k < 4 ? d0[k & 3] : d1[k & 3];
        const float th = mlp_tanh(a + u[k]);
        const float g = on ? d * vh * (1.f - th * th) : 0.f;
        acc += g;
        du[k] += g;
        dv += on ? d * th : 0.f;
      }
      acc_t[t * AM_HC + tid] = acc;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (s0 + k < len) {
        if (nch == 1) duh[((long)(s0 + k) * B + b) * ldduh + h] = from_f<T>(du[k]);
        else duh_part[(((long)ch * S + s0 + k) * B + b) * H + h] = du[k];
      }
  }
  if (nch == 1)
    for (int s = len; s < S; ++s) duh[((long)s * B + b) * ldduh + h] = from_f<T>(0.f);                   // zero at pads
  for (int t = 0; t < nT; ++t) dwq[((long)(t0 + t) * B + b) * lddwq + h] = from_f<T>(acc_t[t * AM_HC + tid]);
  dv_part[((long)b * nch + ch) * H + h] = dv;
}

// duh = the chunks' partials in chunk order, zero at pads (padded rows of the partial slices are never written and never read)
template <class T>
__global__ void __launch_bounds__(256) attn_mlp_bwd_long_fold(const float* __restrict__ part, const long long* __restrict__ lens,
                                                              T* __restrict__ duh, long ldduh, int nch, int B, int S, int H) {
  const long n = (long)S * B * H, i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long row = i / H;
  const int h = (int)(i - row * H), s = (int)(row / B), b = (int)(row - (long)s * B);
  float a = 0.f;
  if (s < (int)lens[b])
    for (int c = 0; c < nch; ++c) a += part[(long)c * n + i];
  duh[row * ldduh + h] = from_f<T>(a);
}

// dHs[s][h] = sum_t P[t][s] dC[t][h] (the direct path only), zero at pads: workgroup (sentence b, columns [c0, c0 + 256), positions
// [sb, sb + 64)).  FAST: 64 queries at a time, P (bf16) [64][64] and dC [64][256] in LDS, both read K-strided; sixteen 32 x 32 tiles, a
// wave owns the column tiles `wave` and `wave + 4` of both position tiles for all of T'.
template <class T, bool FAST>
__global__ void __launch_bounds__(256) attn_mlp_bwd_long_dhs(const T* __restrict__ dcat, long lddc, const float* __restrict__ probs,
                                                             const long long* __restrict__ lens, T* __restrict__ dctx, long lddx, int Tp,
                                                             int B, int S, int H) {
  const int b = blockIdx.x, c0 = blockIdx.y * AM_HC, sb = blockIdx.z * AM_MAXS, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nc = min(AM_HC, H - c0), h = c0 + tid;
  int len = (int)lens[b];
  len = len < S ? len : S;
  if constexpr (FAST) {
    constexpr int PC = AM_HC + 8;
    __shared__ __attribute__((aligned(16))) bf16_t Pb[AM_MAXS * AM_PB];      // [64 queries][AM_PB]
    __shared__ __attribute__((aligned(16))) bf16_t dCs[AM_MAXS * PC];        // [64 queries][PC]
    const int nhc = nc / 32;
    f32x16 c[2][2];                                                          // [column tile wave + 4 i][position tile]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) c[i][j][r] = 0.f;
    const int tEnd = sb < len ? Tp : 0;                                      // a tile of pads only: zeros
    for (int t0 = 0; t0 < tEnd; t0 += AM_MAXS) {
      __syncthreads();                                                       // the previous chunk's fragments are read
      for (int t = wave; t < AM_MAXS; t += 4) {
        const bool on = t0 + t < Tp && sb + lane < len;
        Pb[t * AM_PB + lane] = f2bf(on ? probs[((long)(t0 + t) * B + b) * S + sb + lane] : 0.f);
      }
      stage_rows(dCs, PC, reinterpret_cast<const bf16_t*>(dcat) + ((long)t0 * B + b) * lddc + c0, (long)B * lddc, Tp - t0, AM_MAXS, nc);
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < AM_MAXS / 16; ++ks) {
        const bf16x8 p0 = fragKS(Pb, AM_PB, 0, ks * 16, lane), p1 = fragKS(Pb, AM_PB, 32, ks * 16, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i)
          if (wave + 4 * i < nhc) {
            const bf16x8 d = fragKS(dCs, PC, (wave + 4 * i) * 32, ks * 16, lane);
            c[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p0, d, c[i][0], 0, 0, 0);
            c[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p1, d, c[i][1], 0, 0, 0);
          }
      }
    }
    bf16_t* out = reinterpret_cast<bf16_t*>(dctx);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (wave + 4 * i < nhc)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int srow = sb + 32 * j + acc_row(r, lane);
            if (srow < S) out[((long)srow * B + b) * lddx + c0 + (wave + 4 * i) * 32 + (lane & 31)] = f2bf(srow < len ? c[i][j][r] : 0.f);
          }
  } else if (tid < nc) {
    for (int s0 = sb; s0 < min(sb + AM_MAXS, S); s0 += 8) {
      float dx[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) dx[k] = 0.f;
      for (int t = 0; t < Tp; ++t) {
        const float x = to_f<T>(dcat[((long)t * B + b) * lddc + h]);
        const float* pr = probs + ((long)t * B + b) * S;
#pragma unroll
        for (int k = 0; k < 8; ++k) dx[k] += s0 + k < len ? pr[s0 + k] * x : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (s0 + k < S) dctx[((long)(s0 + k) * B + b) * lddx + h] = from_f<T>(dx[k]);
    }
  }
}

bool rows16(const void* p, long ld) { return (((uintptr_t)p) & 15) == 0 && ld % 8 == 0; }   // 16-byte row loads of bf16

// raises a kernel's dynamic-LDS limit to `bytes` on the CURRENT device (remembered per device: data parallelism may drive several from one
// process); false when the runtime refuses
template <class K>
bool allow_lds(K kernel, size_t bytes, size_t (&have)[64]) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  if (bytes <= have[dev]) return true;
  if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
  have[dev] = bytes;
  return true;
}

}  // namespace
}  // namespace vmmt

extern "C" int vmmt_attn_mlp_fwd(int dtype, const void* wq, int64_t ldwq, const float* bq, const void* uh, int64_t lduh, const float* v,
                                 const void* ctx, int64_t ldc, const int64_t* lens, void* cat, int64_t ldcat, float* probs, int Tp, int B,
                                 int S, int H, void* stream) {
  using namespace vmmt;
  if (!wq || !bq || !uh || !v || !ctx || !lens || !cat || !probs || S <= 0 || S > 64 * AM_LK || H <= 0 || H > 64 * AM_MAXJ || Tp <= 0 || B <= 0)
    return VMMT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VMMT_BF16 && S <= AM_MAXS && H % 32 == 0 && rows16(wq, ldwq) && rows16(uh, lduh) && rows16(ctx, ldc)) {
    const size_t sm = (size_t)((S + 31) & ~31) * (H + 8) * 2 + AM_MAXS * AM_SC * 4 + AM_MAXS * AM_PB * 2;
    static size_t attr[64] = {};
    if (!allow_lds(attn_mlp_fwd_lds, sm, attr)) return VMMT_ELAUNCH;
    int tq = AM_MAXS;                 // queries per workgroup: fewer while the grid leaves compute units without work (restaging uh is cheap)
    while (tq > 16 && (long)B * ((Tp + tq - 1) / tq) < 512) tq >>= 1;
    hipLaunchKernelGGL(attn_mlp_fwd_lds, dim3(B, (Tp + tq - 1) / tq), dim3(256), sm, st, (const bf16_t*)wq, (long)ldwq, bq,
                       (const bf16_t*)uh, (long)lduh, v, (const bf16_t*)ctx, (long)ldc, (const long long*)lens, (bf16_t*)cat, (long)ldcat,
                       probs, Tp, B, S, H, tq);
    return check_launch();
  }
  const unsigned grid = (unsigned)(((long)Tp * B + 3) / 4);
  if (dtype == VMMT_F32)
    hipLaunchKernelGGL(attn_mlp_fwd_wave<float>, dim3(grid), dim3(256), 0, st, (const float*)wq, (long)ldwq, bq, (const float*)uh, (long)lduh,
                       v, (const float*)ctx, (long)ldc, (const long long*)lens, (float*)cat, (long)ldcat, probs, Tp, B, S, H);
  else if (dtype == VMMT_BF16)
    hipLaunchKernelGGL(attn_mlp_fwd_wave<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)wq, (long)ldwq, bq, (const bf16_t*)uh,
                       (long)lduh, v, (const bf16_t*)ctx, (long)ldc, (const long long*)lens, (bf16_t*)cat, (long)ldcat, probs, Tp, B, S, H);
  else return VMMT_EINVAL;
  return check_launch();
}

extern "C" int vmmt_attn_mlp_dv_parts(int B, int H) {
  (void)H;
  return B > 0 ? B : 0;          // one partial row per sentence: the column groups of a sentence own disjoint h
}

extern "C" int vmmt_attn_mlp_bwd(int dtype, const void* dcat, int64_t lddc, const float* probs, const void* wq, int64_t ldwq, const float* bq,
                                 const void* uh, int64_t lduh, const float* v, const void* ctx, int64_t ldc, const int64_t* lens, void* dwq,
                                 int64_t lddwq, void* duh, int64_t ldduh, void* dctx, int64_t lddx, float* dv_part, int Tp, int B, int S,
                                 int H, void* stream) {
  using namespace vmmt;
  if (!dcat || !probs || !wq || !bq || !uh || !v || !ctx || !lens || !dwq || !duh || !dctx || !dv_part || S <= 0 || S > AM_MAXS ||
      Tp <= 0 || Tp > AM_MAXS || H <= 0 || H > 64 * AM_MAXJ || B <= 0)
    return VMMT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(B, (H + AM_HC - 1) / AM_HC);
  const size_t base = (size_t)AM_MAXS * AM_SC * 4 + (size_t)Tp * AM_HC * 4;
  if (dtype == VMMT_BF16 && H % 32 == 0 && rows16(dcat, lddc) && rows16(ctx, ldc)) {
    const size_t sm = base + AM_MAXS * AM_PB * 2 + (size_t)((Tp + 15) & ~15) * (AM_HC + 8) * 2;   // wq columns [T'][256], then dC [ru16(T')][264]
    static size_t attr[64] = {};
    if (!allow_lds(attn_mlp_bwd_kernel<bf16_t, true>, sm, attr)) return VMMT_ELAUNCH;
    hipLaunchKernelGGL((attn_mlp_bwd_kernel<bf16_t, true>), grid, dim3(256), sm, st, (const bf16_t*)dcat, (long)lddc, probs, (const bf16_t*)wq,
                       (long)ldwq, bq, (const bf16_t*)uh, (long)lduh, v, (const bf16_t*)ctx, (long)ldc, (const long long*)lens, (bf16_t*)dwq,
                       (long)lddwq, (bf16_t*)duh, (long)ldduh, (bf16_t*)dctx, (long)lddx, dv_part, Tp, B, S, H);
    return check_launch();
  }
  const size_t sm = base + AM_MAXS * AM_SC * 4;
  if (dtype == VMMT_F32) {
    static size_t attr[64] = {};
    if (!allow_lds(attn_mlp_bwd_kernel<float, false>, sm, attr)) return VMMT_ELAUNCH;
    hipLaunchKernelGGL((attn_mlp_bwd_kernel<float, false>), grid, dim3(256), sm, st, (const float*)dcat, (long)lddc, probs, (const float*)wq,
                       (long)ldwq, bq, (const float*)uh, (long)lduh, v, (const float*)ctx, (long)ldc, (const long long*)lens, (float*)dwq,
                       (long)lddwq, (float*)duh, (long)ldduh, (float*)dctx, (long)lddx, dv_part, Tp, B, S, H);
  } else if (dtype == VMMT_BF16) {
    static size_t attr[64] = {};
    if (!allow_lds(attn_mlp_bwd_kernel<bf16_t, false>, sm, attr)) return VMMT_ELAUNCH;
    hipLaunchKernelGGL((attn_mlp_bwd_kernel<bf16_t, false>), grid, dim3(256), sm, st, (const bf16_t*)dcat, (long)lddc, probs, (const bf16_t*)wq,
                       (long)ldwq, bq, (const bf16_t*)uh, (long)lduh, v, (const bf16_t*)ctx, (long)ldc, (const long long*)lens, (bf16_t*)dwq,
                       (long)lddwq, (bf16_t*)duh, (long)ldduh, (bf16_t*)dctx, (long)lddx, dv_part, Tp, B, S, H);
  } else return VMMT_EINVAL;
  return check_launch();
}

extern "C" int vmmt_attn_mlp_bwd_long_dv_parts(int Tp, int B, int H) {
  (void)H;
  if (Tp <= 0 || B <= 0) return 0;
  const long n = (long)B * ((Tp + vmmt::AM_LTC - 1) / vmmt::AM_LTC);      // one partial row per (sentence, chunk of queries)
  return n <= 0x7fffffffL ? (int)n : 0;
}

extern "C" int vmmt_attn_mlp_bwd_long_scratch(int Tp, int B, int S, int H) {
  if (Tp <= 0 || B <= 0 || S <= 0 || H <= 0) return 0;
  const long nch = (Tp + vmmt::AM_LTC - 1) / vmmt::AM_LTC;
  // dS f32 [T' B][S], then (more than one chunk) the chunks' duh partials f32 [chunks][S B][H]
  const double n = (double)Tp * B * S + (nch > 1 ? (double)nch * S * B * H : 0.0);
  return n <= 2147483647.0 ? (int)n : 0;                                   // 0: beyond what this interface can size
}

extern "C" int vmmt_attn_mlp_bwd_long(int dtype, const void* dcat, int64_t lddc, const float* probs, const void* wq, int64_t ldwq,
                                      const float* bq, const void* uh, int64_t lduh, const float* v, const void* ctx, int64_t ldc,
                                      const int64_t* lens, void* dwq, int64_t lddwq, void* duh, int64_t ldduh, void* dctx, int64_t lddx,
                                      float* dv_part, int Tp, int B, int S, int H, float* scratch, void* stream) {
  using namespace vmmt;
  if (!dcat || !probs || !wq || !bq || !uh || !v || !ctx || !lens || !dwq || !duh || !dctx || !dv_part || !scratch || S <= 0 ||
      S > 64 * AM_LK || Tp <= 0 || H <= 0 || H > 64 * AM_MAXJ || B <= 0 || (dtype != VMMT_BF16 && dtype != VMMT_F32))
    return VMMT_EINVAL;
  const int nq = (Tp + AM_LQ - 1) / AM_LQ, nch = (Tp + AM_LTC - 1) / AM_LTC, nhg = (H + AM_HC - 1) / AM_HC;
  if (nq > 65535 || nch > 65535 || B > 0x7fffffff / nhg || vmmt_attn_mlp_bwd_long_scratch(Tp, B, S, H) <= 0 ||
      vmmt_attn_mlp_bwd_long_dv_parts(Tp, B, H) <= 0)
    return VMMT_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* dS = scratch;
  float* part = scratch + (long)Tp * B * S;
  const long long* ln = (const long long*)lens;
  const bool fast = dtype == VMMT_BF16 && H % 32 == 0 && rows16(dcat, lddc) && rows16(ctx, ldc);
  const size_t sm = (size_t)AM_LTC * ((S + 7) & ~7) * 4 + (size_t)AM_LTC * AM_HC * (dtype == VMMT_BF16 ? 6 : 4);
  const dim3 gq(B, nq), gt(B, nhg, nch), gs(B, nhg, (S + AM_MAXS - 1) / AM_MAXS);
  const unsigned gf = (unsigned)(((long)S * B * H + 255) / 256);
  if (dtype == VMMT_BF16) {
    typedef bf16_t T;
    static size_t attr[64] = {};
    if (!allow_lds(attn_mlp_bwd_long_tanh<T>, sm, attr)) return VMMT_ELAUNCH;
    if (fast)
      hipLaunchKernelGGL((attn_mlp_bwd_long_ds<T, true>), gq, dim3(256), 0, st, (const T*)dcat, (long)lddc, probs, (const T*)ctx, (long)ldc, ln,
                         dS, Tp, B, S, H);
    else
      hipLaunchKernelGGL((attn_mlp_bwd_long_ds<T, false>), gq, dim3(256), 0, st, (const T*)dcat, (long)lddc, probs, (const T*)ctx, (long)ldc,
                         ln, dS, Tp, B, S, H);
    hipLaunchKernelGGL((attn_mlp_bwd_long_tanh<T>), gt, dim3(256), sm, st, dS, (const T*)wq, (long)ldwq, bq, (const T*)uh, (long)lduh, v, ln,
                       (T*)dwq, (long)lddwq, (T*)duh, (long)ldduh, part, dv_part, Tp, B, S, H);
    if (fast)
      hipLaunchKernelGGL((attn_mlp_bwd_long_dhs<T, true>), gs, dim3(256), 0, st, (const T*)dcat, (long)lddc, probs, ln, (T*)dctx, (long)lddx,
                         Tp, B, S, H);
    else
      hipLaunchKernelGGL((attn_mlp_bwd_long_dhs<T, false>), gs, dim3(256), 0, st, (const T*)dcat, (long)lddc, probs, ln, (T*)dctx, (long)lddx,
                         Tp, B, S, H);
    if (nch > 1)
      hipLaunchKernelGGL((attn_mlp_bwd_long_fold<T>), dim3(gf), dim3(256), 0, st, part, ln, (T*)duh, (long)ldduh, nch, B, S, H);
  } else {
    typedef float T;
    static size_t attr[64] = {};
    if (!allow_lds(attn_mlp_bwd_long_tanh<T>, sm, attr)) return VMMT_ELAUNCH;
    hipLaunchKernelGGL((attn_mlp_bwd_long_ds<T, false>), gq, dim3(256), 0, st, (const T*)dcat, (long)lddc, probs, (const T*)ctx, (long)ldc, ln,
                       dS, Tp, B, S, H);
    hipLaunchKernelGGL((attn_mlp_bwd_long_tanh<T>), gt, dim3(256), sm, st, dS, (const T*)wq, (long)ldwq, bq, (const T*)uh, (long)lduh, v, ln,
                       (T*)dwq, (long)lddwq, (T*)duh, (long)ldduh, part, dv_part, Tp, B, S, H);
    hipLaunchKernelGGL((attn_mlp_bwd_long_dhs<T, false>), gs, dim3(256), 0, st, (const T*)dcat, (long)lddc, probs, ln, (T*)dctx, (long)lddx,
                       Tp, B, S, H);
    if (nch > 1)
      hipLaunchKernelGGL((attn_mlp_bwd_long_fold<T>), dim3(gf), dim3(256), 0, st, part, ln, (T*)duh, (long)ldduh, nch, B, S, H);
  }
  return check_launch();
}
