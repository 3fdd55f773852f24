// Fused global-norm clip + SGD / Adagrad / Adadelta over the flat fp32 parameter arena (gfx950, HBM-bound), beside Adam's kernels (optim.hip).
// Reference: onmt/Optim.py:56-67 -> torch.optim.SGD / Adagrad / Adadelta(params, lr=lr), everything else at torch's defaults, behind
// torch.nn.utils.clip_grad_norm(params, max_grad_norm) (Optim.py:94-95):
//   clip_coef = max_norm / (||g||_2 + 1e-6), applied only when < 1 (as optim.hip)
//   SGD       p -= lr g                                                                            (momentum 0, weight decay 0)
//   Adagrad   sum += g^2 ; p -= lr g / (sqrt(sum) + 1e-10)                                         (lr_decay 0; sum starts at adagrad_accum)
//   Adadelta  sq = 0.9 sq + 0.1 g^2 ; d = sqrt(acc + 1e-6) / sqrt(sq + 1e-6) g ; acc = 0.9 acc + 0.1 d^2 ; p -= lr d
// The state lives where Adam's moments live: s1 = flat_m (Adagrad `sum`, Adadelta `square_avg`), s2 = flat_v (Adadelta `acc_delta`).  A kernel
// streams only what its method needs: 12 B per element for SGD, 20 B for Adagrad, 28 B for Adadelta (Adam: 28 B).
#include "common.hpp"
#include "vmmt.h"

namespace vmmt {

// ONE element update per method, shared by the dense kernel and the row-wise kernel below.  Floating-point contraction is off (as for
// adam_elem): a flagged row must come out of the row-wise kernel with the bits the dense kernel gives it, whatever the compiler would like to
// fuse in either place.  The operations and their order are those of torch's single-tensor implementations (addcmul: self + (value * a) * b,
// addcdiv: self + (value * a) / b); sqrtf and the divisions are the correctly rounded ones -- there are no replays here that they could
// slow down, and the dense kernel hides them under its streams.
#pragma clang fp contract(off)
template <int M>
__device__ __forceinline__ void optim_elem(float& p, float ge, float& s1, float& s2, float lr) {
  if constexpr (M == VMMT_OPTIM_SGD) {
    p = p + (-lr) * ge;
  } else if constexpr (M == VMMT_OPTIM_ADAGRAD) {
    s1 = s1 + ge * ge;
    const float sd = sqrtf(s1) + 1e-10f;
    p = p + ((-lr) * ge) / sd;
  } else {
    const float rho = 0.9f, omr = 0.1f, eps = 1e-6f;
    s1 = s1 * rho + (omr * ge) * ge;
    const float sd = sqrtf(s1 + eps);
    const float d = (sqrtf(s2 + eps) / sd) * ge;
    s2 = s2 * rho + (omr * d) * d;
    p = p + (-lr) * d;
  }
}
#pragma clang fp contract(fast)

// the clip coefficient times grad_scale from the norm pieces (slot totals in index order: unused slots hold 0), as adam_kernel forms it
__device__ __forceinline__ float clip_coef(float max_norm, const float* __restrict__ sumsq, float grad_scale) {
  float coef = grad_scale;
  if (max_norm > 0.f) {
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < VMMT_SUMSQ_SLOTS; ++k) ss += sumsq[k];
    const float c = max_norm / (sqrtf(ss) * grad_scale + 1e-6f);
    if (c < 1.f) coef *= c;
  }
  return coef;
}

template <int M> struct Uses {            // which state arrays a method streams
  static constexpr bool S1 = M != VMMT_OPTIM_SGD, S2 = M == VMMT_OPTIM_ADADELTA;
};

// Dense kernel: adam_kernel's shape -- four elements per lane, non-temporal 16-byte streams (read and written once per step: they must not
// push the recurrences' exchange lines and the GEMMs' operands out of the L2s), a grid-stride loop, a scalar path for the range's last 1-3
// elements, the hole of a table the row-wise kernel updates, the bf16 shadow of a sub-range written from the updated registers, the guard
// word first.  (hole_lo, hole_n, sh_lo, sh_n: multiples of 4, see vmmt_adam_step_ranges.)
template <int M>
__global__ void __launch_bounds__(256) optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1, float* __restrict__ s2, long n,
                                                    float lr, float max_norm, const float* __restrict__ sumsq, float grad_scale,
                                                    bf16_t* __restrict__ shadow, int* __restrict__ skip, long sh_lo, long sh_n, long hole_lo, long hole_n) {
  if (skip && __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {      // vmmt.h: the step is not applied
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(skip + 1, 1);
    return;
  }
  const float coef = clip_coef(max_norm, sumsq, grad_scale);
  long j = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (; j < n; j += stride) {
    const long i = j < hole_lo ? j : j + hole_n;          // (logical -> arena index: the hole is skipped)
    const bool sh = shadow && i >= sh_lo && i < sh_lo + sh_n;
    if (j + 3 < n) {
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
      f32x4 pp = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(p + i)), gg = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + i));
      f32x4 aa = z4, bb = z4;
      if constexpr (Uses<M>::S1) aa = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(s1 + i));
      if constexpr (Uses<M>::S2) bb = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(s2 + i));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pp[e], ae = aa[e], be = bb[e];
        optim_elem<M>(pe, gg[e] * coef, ae, be, lr);
        pp[e] = pe; aa[e] = ae; bb[e] = be;
      }
      __builtin_nontemporal_store(pp, reinterpret_cast<f32x4*>(p + i));
      if constexpr (Uses<M>::S1) __builtin_nontemporal_store(aa, reinterpret_cast<f32x4*>(s1 + i));
      if constexpr (Uses<M>::S2) __builtin_nontemporal_store(bb, reinterpret_cast<f32x4*>(s2 + i));
      if (sh) {
        typedef unsigned short us4 __attribute__((ext_vector_type(4)));
        const us4 h = {f2bf(pp[0]), f2bf(pp[1]), f2bf(pp[2]), f2bf(pp[3])};
        *reinterpret_cast<us4*>(shadow + (i - sh_lo)) = h;
      }
    } else {
      for (long k = i; k < i + (n - j); ++k) {              // (the range's last 1-3 elements: behind the hole, if there is one)
        float pk = p[k], ak = 0.f, bk = 0.f;
        if constexpr (Uses<M>::S1) ak = s1[k];
        if constexpr (Uses<M>::S2) bk = s2[k];
        optim_elem<M>(pk, g[k] * coef, ak, bk, lr);
        if constexpr (Uses<M>::S1) s1[k] = ak;
        if constexpr (Uses<M>::S2) s2[k] = bk;
        p[k] = pk;
        if (sh) shadow[k - sh_lo] = f2bf(pk);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Embedding tables by row, SGD and Adagrad.  For both a zero-gradient step is the IDENTITY on parameter and state (p -= lr 0, sum += 0), so a
// row outside the batch needs neither an update nor a replay -- there is nothing "lazy" to catch up on.  The kernel keeps Adam's row
// bookkeeping alive all the same (optim.hip: flags / last / hist), so that rows_mark, rows_catchup, rows_sumsq, the forward plans' catch-up
// entries and the flush in front of checkpoints work on unchanged: the step goes into the ring as one that moved nothing (the entry a
// guard-skipped Adam step leaves: applied = 0), and `last` moves to the step for the flagged and the rolling rows -- data untouched -- so
// that no row falls further behind than the ring is long.  A later catch-up of such a row walks over entries that say "nothing to replay",
// clears the row's gradient and refreshes its bf16 copy, as under Adam.
// Work split as in adam_rows_kernel: a workgroup owns 64 rows, every wave ballots the block's flags with one coalesced load, the waves take
// the flagged rows in turn, a whole row per wave, two 256-column chunks (16 bytes per lane and array) in flight.  g is read for flagged
// rows only; rows without a flag are never loaded.
#define VMMT_LAZY_HDR 4
#define VMMT_ROWS_WAVES 16

template <int M>
__global__ void __launch_bounds__(64 * VMMT_ROWS_WAVES) optim_rows_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1, int R, int C,
                                                                          const int* __restrict__ flags, int* __restrict__ last, int* __restrict__ hist,
                                                                          int step, int roll, float lr, float max_norm, const float* __restrict__ sumsq,
                                                                          float grad_scale, int* __restrict__ skip) {
  const bool skipped = skip && __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float* en = reinterpret_cast<float*>(hist + VMMT_LAZY_HDR + 4 * (step & (VMMT_LAZY_HIST - 1)));
    en[0] = lr; en[1] = 0.f; en[2] = 0.f; en[3] = __int_as_float(step);      // applied = 0: nothing to replay, skipped or not
    hist[0] = step;         // (read by the NEXT forward's mark / catch-up launches only: nothing in this launch looks at it)
    if (skipped) atomicAdd(skip + 1, 1);
  }
  if (skipped) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r0 = blockIdx.x * 64;
  bool hg = false;
  if (r0 + lane < R) {
    hg = flags[(long)(step & 1) * R + r0 + lane] == step;
    // the flagged and the rolling rows are current for this step (wave 0 writes the block's words: one coalesced store)
    if (wave == 0 && (hg || (roll > 0 && (r0 + lane) % roll == step % roll))) last[r0 + lane] = step;
  }
  unsigned long long todo = __ballot(hg);
  if (!todo) return;
  const float coef = clip_coef(max_norm, sumsq, grad_scale);
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; todo; ++k) {
    const int b = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    if (k % VMMT_ROWS_WAVES != wave) continue;
    const long base = (long)(r0 + b) * C;
    for (int cb = 0; cb < C; cb += 512) {
      const int ca = cb + lane * 4, cc = ca + 256;
      const bool la = ca < C, lb = cc < C;
      f32x4 pa = z4, ga = z4, sa = z4, pb = z4, gb = z4, sb = z4;
      if (la) { pa = *reinterpret_cast<f32x4*>(p + base + ca); ga = *reinterpret_cast<const f32x4*>(g + base + ca); }
      if (lb) { pb = *reinterpret_cast<f32x4*>(p + base + cc); gb = *reinterpret_cast<const f32x4*>(g + base + cc); }
      if constexpr (Uses<M>::S1) {
        if (la) sa = *reinterpret_cast<f32x4*>(s1 + base + ca);
        if (lb) sb = *reinterpret_cast<f32x4*>(s1 + base + cc);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pa[e], se = sa[e], unused = 0.f;
        optim_elem<M>(pe, ga[e] * coef, se, unused, lr);
        pa[e] = pe; sa[e] = se;
        pe = pb[e]; se = sb[e];
        optim_elem<M>(pe, gb[e] * coef, se, unused, lr);
        pb[e] = pe; sb[e] = se;
      }
      if (la) *reinterpret_cast<f32x4*>(p + base + ca) = pa;
      if (lb) *reinterpret_cast<f32x4*>(p + base + cc) = pb;
      if constexpr (Uses<M>::S1) {
        if (la) *reinterpret_cast<f32x4*>(s1 + base + ca) = sa;
        if (lb) *reinterpret_cast<f32x4*>(s1 + base + cc) = sb;
      }
    }
  }
}

template <int M>
static int optim_launch(float* p, const float* g, float* s1, float* s2, long n, float lr, float max_norm, const float* sumsq, float grad_scale,
                        int max_blocks, void* shadow_bf16, long sh_lo, long sh_n, long hole_lo, long hole_n, const int32_t* skip, void* stream) {
  long blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;   // throttle: a background update must not saturate HBM
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(optim_kernel<M>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, s1, s2, n, lr, max_norm, sumsq, grad_scale,
                     (bf16_t*)shadow_bf16, const_cast<int*>(skip), sh_lo, sh_n, hole_lo, hole_n);
  return check_launch();
}

}  // namespace vmmt

extern "C" int vmmt_optim_step_ranges(int method, float* p, const float* g, float* s1, float* s2, int64_t span, int64_t hole_lo, int64_t hole_n, float lr,
                                      float max_norm, const float* sumsq, float grad_scale, int max_blocks, void* shadow_bf16, int64_t shadow_lo,
                                      int64_t shadow_n, const int32_t* skip, void* stream) {
  using namespace vmmt;
  if (method != VMMT_OPTIM_SGD && method != VMMT_OPTIM_ADAGRAD && method != VMMT_OPTIM_ADADELTA) return VMMT_EINVAL;
  const bool need1 = method != VMMT_OPTIM_SGD, need2 = method == VMMT_OPTIM_ADADELTA;
  if (!p || !g || (need1 && !s1) || (need2 && !s2) || (max_norm > 0.f && !sumsq)) return VMMT_EINVAL;
  if (span < 0 || hole_lo < 0 || hole_n < 0 || hole_lo + hole_n > span || ((hole_lo | hole_n) & 3)) return VMMT_EINVAL;
  if (shadow_bf16 && (shadow_lo < 0 || shadow_n < 0 || shadow_lo + shadow_n > span || ((shadow_lo | shadow_n) & 3))) return VMMT_EINVAL;
  if (shadow_bf16 && hole_n > 0 && shadow_lo < hole_lo + hole_n && hole_lo < shadow_lo + shadow_n) return VMMT_EINVAL;      // (the shadowed piece lies on one side of the hole)
  if ((((uintptr_t)p) | ((uintptr_t)g) | (need1 ? (uintptr_t)s1 : 0) | (need2 ? (uintptr_t)s2 : 0)) & 15) return VMMT_EINVAL;
  if (((uintptr_t)shadow_bf16) & 7) return VMMT_EINVAL;
  const long n = (long)(span - hole_n), h_lo = hole_n > 0 ? (long)hole_lo : (long)span, s_n = shadow_bf16 ? (long)shadow_n : 0;
  if (n == 0) return VMMT_OK;
  if (method == VMMT_OPTIM_SGD)
    return optim_launch<VMMT_OPTIM_SGD>(p, g, s1, s2, n, lr, max_norm, sumsq, grad_scale, max_blocks, shadow_bf16, (long)shadow_lo, s_n, h_lo, (long)hole_n, skip, stream);
  if (method == VMMT_OPTIM_ADAGRAD)
    return optim_launch<VMMT_OPTIM_ADAGRAD>(p, g, s1, s2, n, lr, max_norm, sumsq, grad_scale, max_blocks, shadow_bf16, (long)shadow_lo, s_n, h_lo, (long)hole_n, skip, stream);
  return optim_launch<VMMT_OPTIM_ADADELTA>(p, g, s1, s2, n, lr, max_norm, sumsq, grad_scale, max_blocks, shadow_bf16, (long)shadow_lo, s_n, h_lo, (long)hole_n, skip, stream);
}

extern "C" int vmmt_optim_rows_step(int method, float* p, const float* g, float* s1, int R, int C, const int32_t* flags, int32_t* last, int32_t* hist, float lr,
                                    int step, int roll, float max_norm, const float* sumsq, float grad_scale, const int32_t* skip, void* stream) {
  using namespace vmmt;
  if (method != VMMT_OPTIM_SGD && method != VMMT_OPTIM_ADAGRAD) return VMMT_EINVAL;        // (Adadelta's state decays on a zero gradient: dense)
  const bool need1 = method == VMMT_OPTIM_ADAGRAD;
  if (!p || !g || (need1 && !s1) || R <= 0 || C <= 0 || C % 4 != 0 || !flags || !last || !hist || step < 1 || roll < 0 || roll > VMMT_LAZY_HIST / 4 ||
      (max_norm > 0.f && !sumsq))
    return VMMT_EINVAL;
  if ((((uintptr_t)p) | ((uintptr_t)g) | (need1 ? (uintptr_t)s1 : 0)) & 15) return VMMT_EINVAL;
  const dim3 grid((unsigned)((R + 63) / 64)), block(64 * VMMT_ROWS_WAVES);
  if (method == VMMT_OPTIM_SGD)
    hipLaunchKernelGGL(optim_rows_kernel<VMMT_OPTIM_SGD>, grid, block, 0, (hipStream_t)stream, p, g, s1, R, C, flags, last, hist, step, roll, lr, max_norm, sumsq,
                       grad_scale, const_cast<int*>(skip));
  else
    hipLaunchKernelGGL(optim_rows_kernel<VMMT_OPTIM_ADAGRAD>, grid, block, 0, (hipStream_t)stream, p, g, s1, R, C, flags, last, hist, step, roll, lr, max_norm,
                       sumsq, grad_scale, const_cast<int*>(skip));
  return check_launch();
}
