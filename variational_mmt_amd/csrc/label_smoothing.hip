// -label_smoothing: the smoothed generator loss as exact low-rank corrections BEHIND the plain generator passes (gfx950, HBM-bound).
// Reference: onmt/Loss.py:146-166 and onmt/VILoss.py:231-243 -- with eps > 0 the criterion is KLDivLoss(sum) against
//   q_m = u on every non-pad column, 1 - eps at y_m, 0 at pad;  u = eps / (V - 2);  q_m = 0 for rows with y_m = pad
// -- and onmt/VILoss.py:479-482 (the reported `elbo` is then minus the summed target log-likelihood alone).
// With s_m = [y_m != pad] inv_norm,  wbar = sum_{j != pad} Wg[j,:],  bbar = sum_{j != pad} b[j],  obar = sum_m s_m o_m,  sigma = sum_m s_m:
//   sum_{j != pad} log p_mj = o_m . wbar + bbar - (V - 1) lse_m
//   loss_m = (1 - eps) ln(1 - eps) + eps ln u + (1 - eps - u) nll_m - u (o_m . wbar + bbar - (V - 1) lse_m)
//   dO_m   = plain dO_m + s_m ((eps + u) Wg[y_m] - u wbar)
//   dWg    = plain dWg + (eps + u) sum_m s_m e_{y_m} (x) o_m - u 1_{!= pad} (x) obar
//   db     = plain db  + (eps + u) sum_m s_m e_{y_m}         - u sigma 1_{!= pad}
// The identities hold whichever way the plain parts were produced (the fused sweep of generator_fused.hip or the G^T path of
// generator.hip), so the sweep, the combine kernels, the dWg product and vmmt_gen_dW_finish are untouched.
//   vmmt_ls_colsum  wbar, bbar: V / rpc row chunks x column blocks of 64 16-byte vectors, one partial row per chunk, folded in chunk order
//   vmmt_ls_rows    one wave per token row, lanes across H in 16-byte vectors: loss_m, dO_m in place, the workgroup's partial of obar / sigma
//                   / the loss sum; a second launch folds the partials in workgroup order
//   vmmt_ls_dW      rank-one part: vocabulary rows cut over workgroups, u obar in LDS, 16-byte read-modify-write; per-token part: one wave per
//                   token adds (eps + u) s_m o_m to row y_m
// Float atomics: ONLY the per-token part of vmmt_ls_dW, exactly where vmmt_gen_dW_finish's one-hot term uses them (several tokens share a
// target row).  Everything else is plain stores over fixed partitions: wbar, bbar, obar, sigma, the loss sum and dO are bit-reproducible.
#include "common.hpp"
#include "vmmt.h"

namespace vmmt {

constexpr int LS_FOLD_WAVES = 16;
constexpr int LS_MAX_H = 1024;            // (the attention kernels' limit as well: Dims)

static int ls_ldp(int H) { return (H + 3) / 4 * 4; }
// rows of Wg per chunk of the column sums: 64, doubled until at most 1024 chunks are left -- a function of V alone
static int ls_rpc(int V) { int r = 64; while ((V + r - 1) / r > 1024) r *= 2; return r; }
static int ls_row_blocks(int M) { const int b = (M + 3) / 4; return b < 1 ? 1 : b > 512 ? 512 : b; }

// out[c] = sum_p part[p][c], c < n: 64 columns per workgroup, wave w adds the partials p = w, w + 16, ... in that order, then the sixteen
// waves' sums are added in wave order.  The launch's LAST workgroup folds scalars instead: out_s[k] = sum_{i < ns, i != skip} src[i sst + k],
// k < ncomp <= 2 (a fixed stride-1024 partition, the wave butterfly, the waves in order).
__global__ void __launch_bounds__(1024) ls_fold_kernel(const float* __restrict__ part, int np, long ldp, int n, float* __restrict__ out,
                                                       const float* __restrict__ src, int ns, int sst, int ncomp, int skip,
                                                       float* __restrict__ out_s) {
  __shared__ float red[LS_FOLD_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (blockIdx.x + 1 < gridDim.x) {
    const int c = blockIdx.x * 64 + lane;
    float a = 0.f;
    if (c < n)
#pragma unroll 4
      for (int p = w; p < np; p += LS_FOLD_WAVES) a += part[(long)p * ldp + c];
    red[w][lane] = a;
    __syncthreads();
    if (w == 0 && c < n) {
      float t = red[0][lane];
#pragma unroll
      for (int k = 1; k < LS_FOLD_WAVES; ++k) t += red[k][lane];
      out[c] = t;
    }
    return;
  }
  // (in fp64: the loss sum of a batch is thousands of row terms of one sign -- one rounding to f32 at the end instead of one per addition)
  __shared__ double reds[LS_FOLD_WAVES][2];
  for (int k = 0; k < ncomp; ++k) {
    double a = 0.0;
    for (int i = threadIdx.x; i < ns; i += 1024)
      if (i != skip) a += (double)src[(long)i * sst + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) reds[w][k] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < ncomp) {
    double t = reds[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < LS_FOLD_WAVES; ++k) t += reds[k][threadIdx.x];
    out_s[threadIdx.x] = (float)t;
  }
}

// part[chunk][c] = sum over the chunk's rows != pad of W[row][c]: the weight is streamed once, 16 bytes per lane and load, four loads in
// flight per lane; the four waves of a workgroup take rows w, w + 4, ... and are added in wave order
template <class T>
__global__ void __launch_bounds__(256) ls_colsum_kernel(const T* __restrict__ W, long ldw, int V, int H, int pad, int rpc,
                                                        float* __restrict__ part, long ldp) {
  constexpr int VEC = 16 / sizeof(T);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c0 = (blockIdx.x * 64 + lane) * VEC;
  const int r0 = blockIdx.y * rpc, r1 = min(V, r0 + rpc);
  float a[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) a[e] = 0.f;
  if (c0 < H) {
    int r = r0 + w;
    for (; r + 12 < r1; r += 16) {
      u32x4 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const u32x4*>(W + (long)(r + 4 * q) * ldw + c0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (r + 4 * q == pad) continue;
        const T* e_ = reinterpret_cast<const T*>(&v[q]);
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] += to_f<T>(e_[e]);
      }
    }
    for (; r < r1; r += 4) {
      if (r == pad) continue;
      const u32x4 v = *reinterpret_cast<const u32x4*>(W + (long)r * ldw + c0);
      const T* e_ = reinterpret_cast<const T*>(&v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) a[e] += to_f<T>(e_[e]);
    }
  }
  __shared__ float red[4][64][VEC + 1];
#pragma unroll
  for (int e = 0; e < VEC; ++e) red[w][lane][e] = a[e];
  __syncthreads();
  if (w == 0)
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      if (c0 + e < H) part[(long)blockIdx.y * ldp + c0 + e] = red[0][lane][e] + red[1][lane][e] + red[2][lane][e] + red[3][lane][e];
}

// One wave per token row (a workgroup's four waves take rows 4 b + w, + 4 gridDim, ...); a lane holds VEC columns of each of PASSES
// column passes (PASSES x 64 x VEC >= H): wbar stays in registers for the whole launch, and so does the wave's partial of obar.
// GRAD = false: the loss alone (validation, Engine.loss): W, dO and part_o are not touched.
template <class T, int PASSES, bool GRAD>
__global__ void __launch_bounds__(256) ls_rows_kernel(const T* __restrict__ O, long ldo, const T* __restrict__ W, long ldw,
                                                      const long long* __restrict__ y, const int* __restrict__ rows, int M, int V, int H,
                                                      int pad, float eps, float u, float inv_norm, const float* __restrict__ lse,
                                                      const float* __restrict__ tok_nll, const float* __restrict__ wbar,
                                                      const float* __restrict__ bbar, float* __restrict__ dO, long lddo,
                                                      float* __restrict__ part_o, long ldp, float* __restrict__ part_s) {
  constexpr int VEC = 16 / sizeof(T);
  constexpr int HP = PASSES * 64 * VEC;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float wb[PASSES][VEC], acc[PASSES][VEC];
#pragma unroll
  for (int p = 0; p < PASSES; ++p)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int c = (p * 64 + lane) * VEC + e;
      wb[p][e] = c < H ? wbar[c] : 0.f;
      acc[p][e] = 0.f;
    }
  // sum_j q ln q of a token row: (1 - eps) ln(1 - eps) + (V - 2) u ln u, with 0 ln 0 = 0
  const float qlnq = (eps < 1.f ? (1.f - eps) * logf(1.f - eps) : 0.f) + (eps > 0.f ? eps * logf(u) : 0.f);
  const float bb = *bbar, ka = eps + u, kn = 1.f - eps - u, vm1 = (float)(V - 1);
  float loss = 0.f, sig = 0.f;
  for (int m = blockIdx.x * 4 + w; m < M; m += gridDim.x * 4) {
    const int r = rows ? rows[m] : m;
    if (r < 0) continue;
    const long long ym = y[r];
    if (ym == pad || ym < 0 || ym >= V) continue;
    u32x4 ov[PASSES], wv[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int c0 = (p * 64 + lane) * VEC;
      ov[p] = c0 < H ? *reinterpret_cast<const u32x4*>(O + (long)r * ldo + c0) : u32x4{0u, 0u, 0u, 0u};
      if constexpr (GRAD) wv[p] = c0 < H ? *reinterpret_cast<const u32x4*>(W + (long)ym * ldw + c0) : u32x4{0u, 0u, 0u, 0u};
    }
    float o[PASSES][VEC], dot = 0.f;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const T* e_ = reinterpret_cast<const T*>(&ov[p]);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        o[p][e] = (p * 64 + lane) * VEC + e < H ? to_f<T>(e_[e]) : 0.f;
        dot = __builtin_fmaf(o[p][e], wb[p][e], dot);
      }
    }
    dot = wave_sum(dot);
    loss += qlnq + kn * tok_nll[r] - u * (dot + bb - vm1 * lse[r]);
    if constexpr (GRAD) {
      sig += inv_norm;
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int c0 = (p * 64 + lane) * VEC;
        const T* e_ = reinterpret_cast<const T*>(&wv[p]);
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {
          if (c0 + 4 * q < H) {
            f32x4* dp = reinterpret_cast<f32x4*>(dO + (long)r * lddo + c0 + 4 * q);
            f32x4 d = *dp;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c0 + 4 * q + e < H) d[e] += inv_norm * (ka * to_f<T>(e_[4 * q + e]) - u * wb[p][4 * q + e]);
            *dp = d;
          }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[p][e] = __builtin_fmaf(inv_norm, o[p][e], acc[p][e]);
      }
    }
  }
  __shared__ float rs[4][2];
  if (lane == 0) { rs[w][0] = loss; rs[w][1] = sig; }
  if constexpr (GRAD) {
    __shared__ float red[4][HP];
#pragma unroll
    for (int p = 0; p < PASSES; ++p)
#pragma unroll
      for (int e = 0; e < VEC; ++e) red[w][(p * 64 + lane) * VEC + e] = acc[p][e];
    __syncthreads();
    for (int c = threadIdx.x; c < H; c += 256) part_o[(long)blockIdx.x * ldp + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
  } else {
    __syncthreads();
  }
  if (threadIdx.x < 2) part_s[blockIdx.x * 2 + threadIdx.x] = rs[0][threadIdx.x] + rs[1][threadIdx.x] + rs[2][threadIdx.x] + rs[3][threadIdx.x];
}

// dWg[v][:] -= u obar, db[v] -= u sigma for the rows v != pad of this workgroup's block of `rpw` vocabulary rows: u obar is staged in LDS
// once, the block's part of the gradient is read and written once, 16 bytes per lane, four vectors in flight
__global__ void __launch_bounds__(256) ls_rank1_kernel(const float* __restrict__ obar, const float* __restrict__ sums, float u, int V, int H,
                                                       int pad, int rpw, float* __restrict__ dW, long lddw, float* __restrict__ db, int vec) {
  __shared__ float so[LS_MAX_H];
  const int tid = threadIdx.x;
  for (int c = tid; c < H; c += 256) so[c] = u * obar[c];
  __syncthreads();
  const int r0 = blockIdx.x * rpw, r1 = min(V, r0 + rpw);
  const float us = u * sums[1];
  for (int r = r0 + tid; r < r1; r += 256)
    if (r != pad) db[r] -= us;
  if (vec) {
    const int nvec = H / 4, total = (r1 - r0) * nvec;
    for (int i0 = tid; i0 < total; i0 += 1024) {
      f32x4 v[4];
      f32x4* ptr[4];
      int col[4];
      bool live[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + 256 * q, ic = i < total ? i : i0;
        const int row = r0 + ic / nvec;
        col[q] = (ic % nvec) * 4;
        live[q] = i < total && row != pad;
        ptr[q] = reinterpret_cast<f32x4*>(dW + (long)row * lddw + col[q]);
        v[q] = *ptr[q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (live[q]) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[q][e] -= so[col[q] + e];
          *ptr[q] = v[q];
        }
    }
  } else {
    const int total = (r1 - r0) * H;
    for (int i = tid; i < total; i += 256) {
      const int row = r0 + i / H, c = i % H;
      if (row != pad) dW[(long)row * lddw + c] -= so[c];
    }
  }
}

// dWg[y_m][:] += coef o_m, db[y_m] += coef, coef = (eps + u) s_m: one wave per token, float atomics (tokens share target rows) -- the shape of
// vmmt_gen_dW_finish's one-hot term, with the coefficient (eps + u) in place of -1
template <class T>
__global__ void __launch_bounds__(256) ls_onehot_kernel(const T* __restrict__ O, long ldo, const long long* __restrict__ y,
                                                        const int* __restrict__ rows, int M, int V, int H, int pad, float coef,
                                                        float* __restrict__ dW, long lddw, float* __restrict__ db) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= M) return;
  const int r = rows ? rows[m] : m;
  if (r < 0) return;
  const long long ym = y[r];
  if (ym == pad || ym < 0 || ym >= V) return;
  float* dst = dW + ym * lddw;
  for (int h = lane; h < H; h += 64) atomicAdd(dst + h, coef * to_f<T>(O[(long)r * ldo + h]));
  if (lane == 0) atomicAdd(db + ym, coef);
}

template <class T>
static bool ls_rows_ok(const void* X, long ld, int H) {
  constexpr int VEC = 16 / sizeof(T);
  return X && (((uintptr_t)X) & 15) == 0 && ld % VEC == 0 && ld >= (long)((H + VEC - 1) / VEC) * VEC;
}

static bool ls_common_ok(int V, int H, int pad, float eps) {
  return V >= 3 && H > 0 && H <= LS_MAX_H && pad >= 0 && pad < V && eps > 0.f && eps <= 1.f;
}

static void ls_fold(const float* part, int np, long ldp, int n, float* out, const float* src, int ns, int sst, int ncomp, int skip, float* out_s,
                    hipStream_t st) {
  hipLaunchKernelGGL(ls_fold_kernel, dim3((unsigned)((n + 63) / 64 + 1)), dim3(1024), 0, st, part, np, ldp, n, out, src, ns, sst, ncomp, skip, out_s);
}

template <class T>
static int ls_colsum_launch(const void* W, long ldw, const float* bias, int V, int H, int pad, float* wbar, float* bbar, float* scratch,
                            hipStream_t st) {
  constexpr int VEC = 16 / sizeof(T);
  if (!ls_rows_ok<T>(W, ldw, H)) return VMMT_EINVAL;
  const int rpc = ls_rpc(V), nch = (V + rpc - 1) / rpc, ldp = ls_ldp(H);
  hipLaunchKernelGGL(ls_colsum_kernel<T>, dim3((unsigned)((H + 64 * VEC - 1) / (64 * VEC)), (unsigned)nch), dim3(256), 0, st, (const T*)W, ldw, V,
                     H, pad, rpc, scratch, (long)ldp);
  ls_fold(scratch, nch, ldp, H, wbar, bias, V, 1, 1, pad, bbar, st);
  return check_launch();
}

template <class T, int PASSES>
static int ls_rows_launch(const void* O, long ldo, const void* W, long ldw, const int64_t* y, const int32_t* rows, int M, int V, int H, int pad,
                          float eps, float inv_norm, const float* lse, const float* tok_nll, const float* wbar, const float* bbar, float* dO,
                          long lddo, float* obar, float* sums, float* scratch, hipStream_t st) {
  const int nb = ls_row_blocks(M), ldp = ls_ldp(H);
  float* part_o = scratch + (long)((V + ls_rpc(V) - 1) / ls_rpc(V)) * ldp;        // (behind the column sums' partials: another stream's)
  float* part_s = part_o + (long)ls_row_blocks(M) * ldp;
  const float u = eps / (float)(V - 2);
  if (dO)
    hipLaunchKernelGGL((ls_rows_kernel<T, PASSES, true>), dim3((unsigned)nb), dim3(256), 0, st, (const T*)O, ldo, (const T*)W, ldw,
                       (const long long*)y, rows, M, V, H, pad, eps, u, inv_norm, lse, tok_nll, wbar, bbar, dO, lddo, part_o, (long)ldp, part_s);
  else
    hipLaunchKernelGGL((ls_rows_kernel<T, PASSES, false>), dim3((unsigned)nb), dim3(256), 0, st, (const T*)O, ldo, (const T*)W, ldw,
                       (const long long*)y, rows, M, V, H, pad, eps, u, inv_norm, lse, tok_nll, wbar, bbar, dO, lddo, part_o, (long)ldp, part_s);
  ls_fold(part_o, nb, ldp, dO ? H : 0, obar, part_s, nb, 2, 2, -1, sums, st);
  return check_launch();
}

template <class T>
static int ls_rows_dispatch(const void* O, long ldo, const void* W, long ldw, const int64_t* y, const int32_t* rows, int M, int V, int H, int pad,
                            float eps, float inv_norm, const float* lse, const float* tok_nll, const float* wbar, const float* bbar, float* dO,
                            long lddo, float* obar, float* sums, float* scratch, hipStream_t st) {
  constexpr int VEC = 16 / sizeof(T);
  if (!ls_rows_ok<T>(O, ldo, H) || (dO && !ls_rows_ok<T>(W, ldw, H))) return VMMT_EINVAL;
  const int np = (H + 64 * VEC - 1) / (64 * VEC);
#define VMMT_LS_ROWS(P) ls_rows_launch<T, P>(O, ldo, W, ldw, y, rows, M, V, H, pad, eps, inv_norm, lse, tok_nll, wbar, bbar, dO, lddo, obar, sums, scratch, st)
  if (np <= 1) return VMMT_LS_ROWS(1);
  if (np <= 2) return VMMT_LS_ROWS(2);
  if (np <= 4) return VMMT_LS_ROWS(4);
#undef VMMT_LS_ROWS
  return VMMT_EINVAL;
}

}  // namespace vmmt

extern "C" int64_t vmmt_ls_ws_floats(int M, int V, int H) {
  using namespace vmmt;
  if (M <= 0 || V <= 0 || H <= 0) return 0;
  const int rpc = ls_rpc(V);
  return (int64_t)((V + rpc - 1) / rpc + ls_row_blocks(M)) * ls_ldp(H) + 2 * ls_row_blocks(M);
}

extern "C" int vmmt_ls_colsum(int dtype, const void* W, int64_t ldw, const float* bias, int V, int H, int pad, float* wbar, float* bbar,
                              float* scratch, void* stream) {
  using namespace vmmt;
  if (!bias || !wbar || !bbar || !scratch || V < 3 || H <= 0 || H > LS_MAX_H || pad < 0 || pad >= V) return VMMT_EINVAL;
  if (dtype == VMMT_F32) return ls_colsum_launch<float>(W, (long)ldw, bias, V, H, pad, wbar, bbar, scratch, (hipStream_t)stream);
  if (dtype == VMMT_BF16) return ls_colsum_launch<bf16_t>(W, (long)ldw, bias, V, H, pad, wbar, bbar, scratch, (hipStream_t)stream);
  return VMMT_EINVAL;
}

extern "C" int vmmt_ls_rows(int dtype, const void* O, int64_t ldo, const void* W, int64_t ldw, const int64_t* y, const int32_t* rows, int M, int V,
                            int H, int pad, float eps, float inv_norm, const float* lse, const float* tok_nll, const float* wbar,
                            const float* bbar, float* dO, int64_t lddo, float* obar, float* sums, float* scratch, void* stream) {
  using namespace vmmt;
  if (!ls_common_ok(V, H, pad, eps) || M <= 0 || !y || !lse || !tok_nll || !wbar || !bbar || !sums || !scratch) return VMMT_EINVAL;
  if (dO && (!obar || (((uintptr_t)dO) & 15) || lddo % 4 != 0 || lddo < (H + 3) / 4 * 4)) return VMMT_EINVAL;
  if (dtype == VMMT_F32)
    return ls_rows_dispatch<float>(O, (long)ldo, W, (long)ldw, y, rows, M, V, H, pad, eps, inv_norm, lse, tok_nll, wbar, bbar, dO, (long)lddo, obar,
                                   sums, scratch, (hipStream_t)stream);
  if (dtype == VMMT_BF16)
    return ls_rows_dispatch<bf16_t>(O, (long)ldo, W, (long)ldw, y, rows, M, V, H, pad, eps, inv_norm, lse, tok_nll, wbar, bbar, dO, (long)lddo, obar,
                                    sums, scratch, (hipStream_t)stream);
  return VMMT_EINVAL;
}

extern "C" int vmmt_ls_dW(int dtype, const void* O, int64_t ldo, const int64_t* y, const int32_t* rows, int M, int V, int H, int pad, float eps,
                          float inv_norm, const float* obar, const float* sums, float* dW, int64_t lddw, float* db, void* stream) {
  using namespace vmmt;
  if (!ls_common_ok(V, H, pad, eps) || M <= 0 || !O || !y || !obar || !sums || !dW || !db || lddw < H || ldo < H) return VMMT_EINVAL;
  if (dtype != VMMT_F32 && dtype != VMMT_BF16) return VMMT_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const float u = eps / (float)(V - 2);
  const int vec = (H % 4 == 0 && lddw % 4 == 0 && (((uintptr_t)dW) & 15) == 0) ? 1 : 0;
  int rpw = 8192 / H;                      // about 2048 16-byte vectors of the gradient per workgroup
  rpw = rpw < 1 ? 1 : rpw;
  hipLaunchKernelGGL(ls_rank1_kernel, dim3((unsigned)((V + rpw - 1) / rpw)), dim3(256), 0, st, obar, sums, u, V, H, pad, rpw, dW, (long)lddw, db, vec);
  const float coef = (eps + u) * inv_norm;
  if (dtype == VMMT_F32)
    hipLaunchKernelGGL(ls_onehot_kernel<float>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, (const float*)O, (long)ldo, (const long long*)y, rows,
                       M, V, H, pad, coef, dW, (long)lddw, db);
  else
    hipLaunchKernelGGL(ls_onehot_kernel<bf16_t>, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, (const bf16_t*)O, (long)ldo, (const long long*)y,
                       rows, M, V, H, pad, coef, dW, (long)lddw, db);
  return check_launch();
}
