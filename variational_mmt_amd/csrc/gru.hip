// GRU time-step kernels (forward and backward) for gfx950: -rnn_type GRU.
//
// The reference builds every recurrence with getattr(nn, rnn_type) (encoder: onmt/Models.py:124-129,140-147 with packed
// sequences; decoder: onmt/VI_Model1.py:137-152), so -rnn_type GRU runs cuDNN's GRU there.  Here, as for the LSTM (lstm.hip),
// the input projection of the whole sequence is one GEMM and only the sequential part runs per time step, one launch per
// step, both directions of a bidirectional layer in one launch (blockIdx.z).  torch's nn.GRU, gate order r, z, n:
//     r = sigmoid(gx_r + h W_hr^T)      z = sigmoid(gx_z + h W_hz^T)      hn = h W_hn^T + b_hn
//     n = tanh(gx_n + r * hn)           h' = n + z * (h - n)
// The reset gate sits INSIDE the candidate's non-linearity, which is what keeps this from being lstm.hip with a gate fewer:
//   * b_hn cannot be folded into gx (it is scaled by r): it is an operand of the step;
//   * the recurrent product's n column stays apart from gx_n until r is known;
//   * the backward has TWO gate-gradient matrices: the input side (dW_ih, db_ih, dx) sees [dr, dz, dn], the recurrent side
//     (dW_hh, db_hh, dh_prev) sees [dr, dz, dn * r].  Both are written in full ([B][3H] each): the weight-gradient GEMMs and the
//     next step's recurrent product then read plain matrices.
// A GRU has no cell state: the state IS the output row, so h_prev of step t is h_out of the step before (zero at padded
// positions, which is exactly what starts the reverse direction from zero at a sentence's last token), and the f32 carry of the
// backward is the direct path dh_{t+1} * z_{t+1}.
// Saved for the backward, in T: r, z, n and hn (columns g * H + u of one [B][4H] row); h_prev is re-read from the outputs.
//
// bf16 fast kernels -- the work split, and why it is not the LSTM's.
//   A workgroup owns 32 sentences x 16 hidden units (256 workgroups at B = 256, H = 512: one per CU) and has 8 waves.
//   The LSTM kernels split their waves 2 row halves x 4 K quarters: every wave reads each B fragment (W_hh rows out of LDS) for
//   ONE 16-row half.  With three gate tiles instead of four the LDS image of a 512-deep chunk is 48 rows x 1 KiB = 48 KiB, and
//   exactly as large as a fold buffer of 8 K slices x 2 row halves x 3 gates x 4 registers x 64 lanes of f32 -- so here the
//   8 waves are 8 K SLICES (k-step s belongs to wave s % 8) and every wave multiplies BOTH row halves: each ds_read_b128 of a
//   W_hh fragment feeds two MFMAs, 6 fragment reads and 12 v_mfma_f32_16x16x32_bf16 per wave at H = 512 where the LSTM split
//   would need 12 reads for the same 12 MFMAs.  The price is a deeper fold (8 partial sums per gate instead of 4), paid in
//   conflict-free lane-contiguous LDS reads.  The backward (K = 3H, the three gate blocks of a W_hh^T row staged side by side:
//   16 rows x 3 KiB) uses the same split: 48 k-steps over 8 waves, 6 fragment reads and 12 MFMAs per wave.
//   K is staged in chunks of KC = the smallest power of two >= H, at most 512 (rounds of 512 beyond); a chunk need not divide H, the
//   k-steps at or beyond H are neither staged nor multiplied (H = 96 runs one 128-wide round with 3 of its 4 k-steps).
//   W_hh rows come by LDS-DMA (global_load_lds_dwordx4), unpadded and XOR-swizzled on the SOURCE side as in lstm.hip; h_prev /
//   dgh_next go straight from global memory into A fragments.  The C layout of the 16x16 MFMA (col = lane & 15,
//   row = 4 * (lane >> 4) + reg) puts r, z and hn of one hidden unit into the same lane; after the fold wave w finishes register
//   w >> 1 of row half w & 1, i.e. every lane exactly one (sentence, unit) cell, lane-local.
// Plain templates (f32, H % 32 != 0, unaligned rows) reuse the block GEMM main loop of common.hpp with three gate tiles.
//
// Not built: a persistent one-launch-per-sequence GRU (the counterpart of lstm_seq.hip); the chain of per-step launches is the
// product path.
#include "common.hpp"
#include "vmmt.h"

namespace vmmt {

struct GruDirF {
  const void* h_prev; long ld_hprev;     // T [B][ld]
  const void* w_hh; long ld_w;           // T [3H][ld] (k contiguous), rows r | z | n
  const float* gx; long ld_gx;           // f32 [B][ld]: x W_ih^T + b_ih (+ b_hh's r and z parts), columns g * H + u
  const float* gx2; long ld_gx2;         // f32 [B][ld] or null: per-sentence addend
  const float* b_hn;                     // f32 [H]
  void* saved; long ld_saved;            // T [B][ld]: r, z, n, hn at columns g * H + u
  void* h_out; long ld_h;                // T [B][ld] (zero at pads)
  void* h_n; long ld_hn;                 // T [B][ld] or null: final state capture
  int t, capture;
};
struct GruArgsF { GruDirF d[2]; const long long* lens; int B, H; };

struct GruDirB {
  const void* dgh_next; long ld_dgn;     // T [B][ld] recurrent-side gate gradients of the step processed before, or null
  const void* w_hh_t; long ld_wt;        // T [H][ld]: W_hh transposed (k = gate row index contiguous, 3H)
  const void* dh_above; long ld_dha;     // T or null
  const void* saved; long ld_saved;      // T r, z, n, hn of step t
  const void* h_prev; long ld_hp;        // T state that entered step t (null = zeros)
  float* dh_carry; long ld_dhc;          // f32 in/out: dh_{t+1} z_{t+1}
  void* dgx_out; long ld_dgx;            // T [B][ld]: dr, dz, dn
  void* dgh_out; long ld_dgh;            // T [B][ld]: dr, dz, dn * r
  const float* dh_n; long ld_dhn;        // f32 or null
  float* dh0_out; long ld_dh0;           // f32, mode 1
  int t, inject;
};
struct GruArgsB { GruDirB d[2]; const long long* lens; int B, H, mode; };

// the cell of one (sentence, hidden unit); shared by the plain and the fast kernels (the fused multiply-adds are spelled out)
struct GruCell { float r, z, n, hn, h; };
__device__ __forceinline__ GruCell gru_cell_math(float pr, float pz, float gxn, float acc_n, float bhn, float hp) {
  GruCell c;
  c.r = cell_sigmoid_(pr); c.z = cell_sigmoid_(pz);
  c.hn = acc_n + bhn;
  c.n = cell_tanh_(__builtin_fmaf(c.r, c.hn, gxn));
  c.h = __builtin_fmaf(c.z, hp - c.n, c.n);
  return c;
}
struct GruCellGrad { float dr, dz, dn, dnr, carry; };
__device__ __forceinline__ GruCellGrad gru_cell_bwd_math(float r, float z, float n, float hn, float hp, float dh) {
  GruCellGrad g;
  g.dn = dh * (1.f - z) * __builtin_fmaf(-n, n, 1.f);
  g.dz = dh * (hp - n) * z * (1.f - z);
  g.dr = g.dn * hn * r * (1.f - r);
  g.dnr = g.dn * r;
  g.carry = dh * z;
  return g;
}

struct GruInF { float gr, gz, gn, bhn, hp; long long len; };
template <class T>
__device__ __forceinline__ GruInF gru_fwd_load(const GruDirF& d, const long long* lens, int b, int u, int H, int B) {
  GruInF in;
  const long bb = b < B ? b : 0;
  const float* gx = d.gx + bb * d.ld_gx + u;
  in.gr = gx[0]; in.gz = gx[H]; in.gn = gx[2 * (long)H];
  if (d.gx2) {
    const float* g2 = d.gx2 + bb * d.ld_gx2 + u;
    in.gr += g2[0]; in.gz += g2[H]; in.gn += g2[2 * (long)H];
  }
  in.bhn = d.b_hn[u];
  in.hp = to_f<T>(reinterpret_cast<const T*>(d.h_prev)[bb * d.ld_hprev + u]);
  in.len = lens ? lens[bb] : 0;
  return in;
}
template <class T>
__device__ __forceinline__ void gru_fwd_apply(const GruDirF& d, bool has_lens, const GruInF& in, int b, int u, int H, float pr,
                                              float pz, float pn) {
  const GruCell c = gru_cell_math(pr + in.gr, pz + in.gz, in.gn, pn, in.bhn, in.hp);
  const bool valid = !has_lens || d.t < in.len;
  T* sv = reinterpret_cast<T*>(d.saved) + (long)b * d.ld_saved + u;
  sv[0] = from_f<T>(c.r); sv[H] = from_f<T>(c.z); sv[2 * (long)H] = from_f<T>(c.n); sv[3 * (long)H] = from_f<T>(c.hn);
  reinterpret_cast<T*>(d.h_out)[(long)b * d.ld_h + u] = from_f<T>(valid ? c.h : 0.f);
  const bool cap = d.capture == 3 || (d.capture == 1 && d.t == in.len - 1) || (d.capture == 2 && d.t == 0);
  if (cap && d.h_n) reinterpret_cast<T*>(d.h_n)[(long)b * d.ld_hn + u] = from_f<T>(c.h);
}

struct GruInB { float r, z, n, hn, hp, dha, dhc, dhn; long long len; };
template <class T>
__device__ __forceinline__ GruInB gru_bwd_load(const GruDirB& d, const long long* lens, int b, int u, int H, int B) {
  GruInB in;
  const long bb = b < B ? b : 0;
  const T* sv = reinterpret_cast<const T*>(d.saved) + bb * d.ld_saved + u;
  in.r = to_f<T>(sv[0]); in.z = to_f<T>(sv[H]); in.n = to_f<T>(sv[2 * (long)H]); in.hn = to_f<T>(sv[3 * (long)H]);
  in.hp = d.h_prev ? to_f<T>(reinterpret_cast<const T*>(d.h_prev)[bb * d.ld_hp + u]) : 0.f;
  in.dha = d.dh_above ? to_f<T>(reinterpret_cast<const T*>(d.dh_above)[bb * d.ld_dha + u]) : 0.f;
  in.dhc = d.dh_carry[bb * d.ld_dhc + u];
  in.dhn = d.dh_n ? d.dh_n[bb * d.ld_dhn + u] : 0.f;
  in.len = lens ? lens[bb] : 0;
  return in;
}
// dh = dgh_next W_hh (the recurrent term) on entry
template <class T>
__device__ __forceinline__ void gru_bwd_apply(const GruDirB& d, bool has_lens, const GruInB& in, int b, int u, int H, float dh) {
  const bool valid = !has_lens || d.t < in.len;
  T* gxo = reinterpret_cast<T*>(d.dgx_out) + (long)b * d.ld_dgx + u;
  T* gho = reinterpret_cast<T*>(d.dgh_out) + (long)b * d.ld_dgh + u;
  float* dhc = d.dh_carry + (long)b * d.ld_dhc + u;
  if (!valid) {
    gxo[0] = T(0); gxo[H] = T(0); gxo[2 * (long)H] = T(0);
    gho[0] = T(0); gho[H] = T(0); gho[2 * (long)H] = T(0);
    *dhc = 0.f;
    return;
  }
  dh += in.dha + in.dhc;
  const bool inj = d.inject == 3 || (d.inject == 1 && d.t == in.len - 1) || (d.inject == 2 && d.t == 0);
  if (inj) dh += in.dhn;
  const GruCellGrad g = gru_cell_bwd_math(in.r, in.z, in.n, in.hn, in.hp, dh);
  const T dr = from_f<T>(g.dr), dz = from_f<T>(g.dz);
  gxo[0] = dr; gxo[H] = dz; gxo[2 * (long)H] = from_f<T>(g.dn);
  gho[0] = dr; gho[H] = dz; gho[2 * (long)H] = from_f<T>(g.dnr);
  *dhc = g.carry;
}
// mode 1: the gradient of the initial state = recurrent term + direct path
__device__ __forceinline__ void gru_dh0(const GruDirB& d, int b, int u, float dh) {
  if (d.dh_carry) dh += d.dh_carry[(long)b * d.ld_dhc + u];
  d.dh0_out[(long)b * d.ld_dh0 + u] = dh;
}

// ------------------------------------------------------------------------------------------------------------
// plain kernels: any T, any H, any alignment.  64 sentences x 32 units per workgroup, two waves, three 32 x 32 gate tiles each.
// ------------------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(128) gru_step_fwd_kernel(GruArgsF a) {
  constexpr int BK = 32, NT = 128, BM = 64, BU = 32, BN = 3 * BU;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  const GruDirF& d = a.d[blockIdx.z];
  const int B = a.B, H = a.H;
  const int m0 = blockIdx.x * BM, u0 = blockIdx.y * BU;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int aoff[1] = {wave * 32};
  int boff[3] = {0, BU, 2 * BU};
  f32x16 acc[1][3];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][g][r] = 0.f;
  LinearMap amap{m0, B};
  GateMap bmap{u0, H, BU};
  gemm_mainloop<T, BM, BN, BK, NT, true, true, 1, 3>((const T*)d.h_prev, d.ld_hprev, amap, (const T*)d.w_hh, d.ld_w,
                                                      bmap, H, 0, 0, aoff, boff, acc, smem);
  const int u = u0 + (lane & 31);
  if (u >= H) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int b = m0 + aoff[0] + acc_row(r, lane);
    if (b >= B) continue;
    const GruInF in = gru_fwd_load<T>(d, a.lens, b, u, H, B);
    gru_fwd_apply<T>(d, a.lens != nullptr, in, b, u, H, acc[0][0][r], acc[0][1][r], acc[0][2][r]);
  }
}

template <class T>
__global__ void __launch_bounds__(256) gru_step_bwd_kernel(GruArgsB a) {
  constexpr int BK = 32, NT = 256, BM = 64, BN = 64;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* smem = reinterpret_cast<T*>(smem_raw);
  const GruDirB& d = a.d[blockIdx.z];
  const int B = a.B, H = a.H;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int aoff[1] = {(wave >> 1) * 32};
  int boff[1] = {(wave & 1) * 32};
  f32x16 acc[1][1];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
  if (d.dgh_next) {
    LinearMap amap{m0, B}, bmap{n0, H};
    gemm_mainloop<T, BM, BN, BK, NT, true, true, 1, 1>((const T*)d.dgh_next, d.ld_dgn, amap, (const T*)d.w_hh_t, d.ld_wt,
                                                        bmap, 3 * H, 0, 0, aoff, boff, acc, smem);
  }
  const int u = n0 + boff[0] + (lane & 31);
  if (u >= H) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int b = m0 + aoff[0] + acc_row(r, lane);
    if (b >= B) continue;
    if (a.mode == 1) { gru_dh0(d, b, u, acc[0][0][r]); continue; }
    const GruInB in = gru_bwd_load<T>(d, a.lens, b, u, H, B);
    gru_bwd_apply<T>(d, a.lens != nullptr, in, b, u, H, acc[0][0][r]);
  }
}

// ==============================================================================================================
// bf16 fast kernels (see the header comment for the split)
// ==============================================================================================================
constexpr int GRU_FOLD_F = 8 * 2 * 3 * 4 * 64 * 4;      // forward fold buffer: [slice][half][gate][reg][lane] f32 = 48 KiB
constexpr int GRU_FOLD_B = 8 * 2 * 4 * 64 * 4;          // backward: [slice][half][reg][lane] f32 = 16 KiB

// forward: 48 staged rows (gate r >> 4, unit r & 15) of KC elements
template <int KC> struct GruFwdCfg {
  static constexpr int ROWB = KC * 2;                          // bytes per staged row
  static constexpr int NCH = ROWB / 16;                        // 16-byte chunks per row (<= 64)
  static constexpr int RPB = ROWB >= 256 ? 1 : 256 / ROWB;     // rows per 256-byte bank row
  static constexpr int KMASK = (NCH < 16 ? NCH : 16) - 1;
  static constexpr int NKS = KC / 32;                          // MFMA k-steps per chunk
  static constexpr int PER = (NKS + 7) / 8;                    // k-steps per wave
  static constexpr int LDS = 48 * ROWB > GRU_FOLD_F ? 48 * ROWB : GRU_FOLD_F;
  static __device__ __forceinline__ int key(int row) { return (row / RPB) & KMASK; }
};

template <int KC>
__global__ void __launch_bounds__(512) gru_step_fwd_fast(GruArgsF a) {
  using Cf = GruFwdCfg<KC>;
  constexpr int ROWB = Cf::ROWB, PER = Cf::PER;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const GruDirF& d = a.d[blockIdx.z];
  const int B = a.B, H = a.H;
  const int m0 = blockIdx.x * 32, u0 = blockIdx.y * 16;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n = lane & 15, kg = lane >> 4;
  const int fh = wave & 1, fr = wave >> 1;                         // the cell this lane finishes: row half fh, register fr
  const int brow = m0 + fh * 16 + kg * 4 + fr, u = u0 + n;
  f32x4_t acc[2][3];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[h][g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const char* wp = reinterpret_cast<const char*>(d.w_hh);
  const char* ap[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
    ap[h] = reinterpret_cast<const char*>(d.h_prev) + ((long)min(m0 + h * 16 + n, B - 1) * d.ld_hprev + kg * 8) * 2;
  GruInF in;
  for (int k0 = 0; k0 < H; k0 += KC) {
    if (k0 > 0) __syncthreads();
    const int kleft = H - k0;                                       // a chunk need not divide H: its tail is neither staged nor multiplied
    if (lane < Cf::NCH) {
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const int r = wave + 8 * j;                                 // staged row: gate r >> 4, unit u0 + (r & 15)
        const long row = (long)(r >> 4) * H + u0 + (r & 15);
        const int sc = lane ^ Cf::key(r);                           // source chunk of this lane's LDS slot
        if (sc * 8 < kleft) dma16(wp + (row * d.ld_w + k0) * 2 + sc * 16, lds + r * ROWB);
      }
    }
    u32x4 af[2][PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int s = wave + 8 * q;                                   // this wave's k-steps: s, s + 8, ...
      if (s < Cf::NKS && s * 32 < kleft) {
#pragma unroll
        for (int h = 0; h < 2; ++h) af[h][q] = *reinterpret_cast<const u32x4*>(ap[h] + (long)(k0 + s * 32) * 2);
      }
    }
    if (k0 == 0) in = gru_fwd_load<bf16_t>(d, a.lens, brow, u, H, B);
    __syncthreads();                                                // drains vmcnt(0): every piece has landed
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int s = wave + 8 * q;
      if (s < Cf::NKS && s * 32 < kleft) {
        const int c = s * 4 + kg;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          const int row = g * 16 + n;
          const bf16x8 bv = *reinterpret_cast<const bf16x8*>(lds + row * ROWB + ((c ^ Cf::key(row)) * 16));
#pragma unroll
          for (int h = 0; h < 2; ++h)
            acc[h][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[h][q]), bv, acc[h][g], 0, 0, 0);
        }
      }
    }
  }
  // fold the eight K slices through LDS; every lane then finishes ONE (sentence, unit) cell
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);                      // [slice][half][gate][reg][lane]
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(((wave * 2 + h) * 3 + g) * 4 + r) * 64 + lane] = acc[h][g][r];
  __syncthreads();
  if (brow < B) {
    float p[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      p[g] = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) p[g] += red[(((w * 2 + fh) * 3 + g) * 4 + fr) * 64 + lane];
    }
    gru_fwd_apply<bf16_t>(d, a.lens != nullptr, in, brow, u, H, p[0], p[1], p[2]);
  }
}

// backward: 16 staged rows of W_hh^T, each the three gate blocks' KC-element segments side by side
template <int KC> struct GruBwdCfg {
  static constexpr int SEGB = KC * 2;                          // bytes per gate segment
  static constexpr int ROWB = 3 * SEGB;
  static constexpr int NCH = SEGB / 16;                        // chunks per segment (<= 64)
  static constexpr int KMASK = (NCH < 16 ? NCH : 16) - 1;
  static constexpr int NKS = KC / 32;                          // k-steps per segment
  static constexpr int PER = (3 * NKS + 7) / 8;                // k-steps per wave
  static constexpr int LDS = 16 * ROWB > GRU_FOLD_B ? 16 * ROWB : GRU_FOLD_B;
  static __device__ __forceinline__ int key(int row) { return row & KMASK; }
};

template <int KC>
__global__ void __launch_bounds__(512) gru_step_bwd_fast(GruArgsB a) {
  using Cf = GruBwdCfg<KC>;
  constexpr int ROWB = Cf::ROWB, SEGB = Cf::SEGB, PER = Cf::PER, NKS = Cf::NKS;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const GruDirB& d = a.d[blockIdx.z];
  const int B = a.B, H = a.H;
  const int m0 = blockIdx.x * 32, u0 = blockIdx.y * 16;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n = lane & 15, kg = lane >> 4;
  const int fh = wave & 1, fr = wave >> 1;
  const int brow = m0 + fh * 16 + kg * 4 + fr, u = u0 + n;
  GruInB in;
  f32x4_t acc[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
  if (d.dgh_next) {
    const char* wp = reinterpret_cast<const char*>(d.w_hh_t);
    const char* ap[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
      ap[h] = reinterpret_cast<const char*>(d.dgh_next) + ((long)min(m0 + h * 16 + n, B - 1) * d.ld_dgn + kg * 8) * 2;
    for (int k0 = 0; k0 < H; k0 += KC) {
      if (k0 > 0) __syncthreads();
      const int kleft = H - k0;
      if (lane < Cf::NCH) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const int p = wave + 8 * j;                               // piece: row p / 3, gate block p % 3
          const int r = p / 3, g = p % 3;
          const int sc = lane ^ Cf::key(r);
          if (sc * 8 < kleft) dma16(wp + ((long)(u0 + r) * d.ld_wt + (long)g * H + k0) * 2 + sc * 16, lds + r * ROWB + g * SEGB);
        }
      }
      u32x4 af[2][PER];
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        const int s = wave + 8 * q;                                 // k-step s: gate block s / NKS, step s % NKS inside it
        if (s < 3 * NKS && (s % NKS) * 32 < kleft) {
          const long k = (long)(s / NKS) * H + k0 + (s % NKS) * 32;
#pragma unroll
          for (int h = 0; h < 2; ++h) af[h][q] = *reinterpret_cast<const u32x4*>(ap[h] + k * 2);
        }
      }
      if (k0 == 0 && a.mode == 0) in = gru_bwd_load<bf16_t>(d, a.lens, brow, u, H, B);
      __syncthreads();
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        const int s = wave + 8 * q;
        if (s < 3 * NKS && (s % NKS) * 32 < kleft) {
          const int c = (s % NKS) * 4 + kg;
          const bf16x8 bv = *reinterpret_cast<const bf16x8*>(lds + n * ROWB + (s / NKS) * SEGB + ((c ^ Cf::key(n)) * 16));
#pragma unroll
          for (int h = 0; h < 2; ++h)
            acc[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[h][q]), bv, acc[h], 0, 0, 0);
        }
      }
    }
  } else if (a.mode == 0) {
    in = gru_bwd_load<bf16_t>(d, a.lens, brow, u, H, B);
  }
  __syncthreads();
  float* red = reinterpret_cast<float*>(lds);                      // [slice][half][reg][lane]
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[((wave * 2 + h) * 4 + r) * 64 + lane] = acc[h][r];
  __syncthreads();
  if (brow < B) {
    float dh = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) dh += red[((w * 2 + fh) * 4 + fr) * 64 + lane];
    if (a.mode == 1) gru_dh0(d, brow, u, dh);
    else gru_bwd_apply<bf16_t>(d, a.lens != nullptr, in, brow, u, H, dh);
  }
}

// the smallest chunk in {32, ..., 512} that holds a whole row; above 512 rounds of 512.  The chunk need not divide H (96 -> 128, 160 -> 256,
// 544 -> 512 + a 32-deep tail round): the kernels stage and multiply only the k-steps below H
static int gru_chunk(int H) { for (int kc = 32; kc < 512; kc <<= 1) if (kc >= H) return kc; return 512; }

template <int KC>
static int gru_launch_fwd_fast(const GruArgsF& a, int ndir, hipStream_t st) {
  hipLaunchKernelGGL(gru_step_fwd_fast<KC>, dim3((a.B + 31) / 32, a.H / 16, ndir), dim3(512), GruFwdCfg<KC>::LDS, st, a);
  return check_launch();
}
template <int KC>
static int gru_launch_bwd_fast(const GruArgsB& a, int ndir, hipStream_t st) {
  hipLaunchKernelGGL(gru_step_bwd_fast<KC>, dim3((a.B + 31) / 32, a.H / 16, ndir), dim3(512), GruBwdCfg<KC>::LDS, st, a);
  return check_launch();
}

static void fill_f(GruDirF& o, const vmmt_gru_dir_fwd& i) {
  o.h_prev = i.h_prev; o.ld_hprev = i.ld_hprev; o.w_hh = i.w_hh; o.ld_w = i.ld_w; o.gx = (const float*)i.gx; o.ld_gx = i.ld_gx;
  o.gx2 = (const float*)i.gx2; o.ld_gx2 = i.ld_gx2; o.b_hn = (const float*)i.b_hn; o.saved = i.saved; o.ld_saved = i.ld_saved;
  o.h_out = i.h_out; o.ld_h = i.ld_h; o.h_n = i.h_n; o.ld_hn = i.ld_hn; o.t = i.t; o.capture = i.capture;
}
static void fill_b(GruDirB& o, const vmmt_gru_dir_bwd& i) {
  o.dgh_next = i.dgh_next; o.ld_dgn = i.ld_dgn; o.w_hh_t = i.w_hh_t; o.ld_wt = i.ld_wt; o.dh_above = i.dh_above; o.ld_dha = i.ld_dha;
  o.saved = i.saved; o.ld_saved = i.ld_saved; o.h_prev = i.h_prev; o.ld_hp = i.ld_hp; o.dh_carry = (float*)i.dh_carry; o.ld_dhc = i.ld_dhc;
  o.dgx_out = i.dgx_out; o.ld_dgx = i.ld_dgx; o.dgh_out = i.dgh_out; o.ld_dgh = i.ld_dgh; o.dh_n = (const float*)i.dh_n; o.ld_dhn = i.ld_dhn;
  o.dh0_out = (float*)i.dh0_out; o.ld_dh0 = i.ld_dh0; o.t = i.t; o.inject = i.inject;
}

}  // namespace vmmt


extern "C" int vmmt_gru_step_fwd(int dtype, int ndir, const vmmt_gru_dir_fwd* dirs, const int64_t* lens, int B, int H,
                                 void* stream) {
  using namespace vmmt;
  if (ndir < 1 || ndir > 2 || !dirs || B <= 0 || H <= 0 || (dtype != VMMT_F32 && dtype != VMMT_BF16)) return VMMT_EINVAL;
  GruArgsF a;
  for (int k = 0; k < ndir; ++k) {
    if (!dirs[k].h_prev || !dirs[k].w_hh || !dirs[k].gx || !dirs[k].b_hn || !dirs[k].saved || !dirs[k].h_out) return VMMT_EINVAL;
    fill_f(a.d[k], dirs[k]);
  }
  if (ndir == 1) a.d[1] = a.d[0];
  a.lens = (const long long*)lens; a.B = B; a.H = H;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VMMT_BF16 && H % 32 == 0) {
    bool ok = true;
    for (int k = 0; k < ndir; ++k) ok = ok && al16(dirs[k].h_prev, dirs[k].ld_hprev) && al16(dirs[k].w_hh, dirs[k].ld_w);
    if (ok) {
      switch (gru_chunk(H)) {
        case 512: return gru_launch_fwd_fast<512>(a, ndir, st);
        case 256: return gru_launch_fwd_fast<256>(a, ndir, st);
        case 128: return gru_launch_fwd_fast<128>(a, ndir, st);
        case 64: return gru_launch_fwd_fast<64>(a, ndir, st);
        default: return gru_launch_fwd_fast<32>(a, ndir, st);
      }
    }
  }
  dim3 grid((B + 63) / 64, (H + 31) / 32, ndir);
  if (dtype == VMMT_F32) {
    size_t sm = gemm_smem_elems<float, 64, 96, 32>() * sizeof(float);
    hipLaunchKernelGGL(gru_step_fwd_kernel<float>, grid, dim3(128), sm, st, a);
  } else {
    size_t sm = gemm_smem_elems<bf16_t, 64, 96, 32>() * sizeof(bf16_t);
    hipLaunchKernelGGL(gru_step_fwd_kernel<bf16_t>, grid, dim3(128), sm, st, a);
  }
  return check_launch();
}

extern "C" int vmmt_gru_step_bwd(int dtype, int ndir, const vmmt_gru_dir_bwd* dirs, const int64_t* lens, int B, int H,
                                 int mode, void* stream) {
  using namespace vmmt;
  if (ndir < 1 || ndir > 2 || !dirs || B <= 0 || H <= 0 || mode < 0 || mode > 1 || (dtype != VMMT_F32 && dtype != VMMT_BF16))
    return VMMT_EINVAL;
  GruArgsB a;
  for (int k = 0; k < ndir; ++k) {
    const vmmt_gru_dir_bwd& i = dirs[k];
    if (mode == 1 && (!i.dgh_next || !i.dh0_out)) return VMMT_EINVAL;
    if (mode == 0 && (!i.saved || !i.dh_carry || !i.dgx_out || !i.dgh_out)) return VMMT_EINVAL;
    if (i.dgh_next && !i.w_hh_t) return VMMT_EINVAL;
    fill_b(a.d[k], i);
  }
  if (ndir == 1) a.d[1] = a.d[0];
  a.lens = (const long long*)lens; a.B = B; a.H = H; a.mode = mode;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VMMT_BF16 && H % 32 == 0) {
    bool ok = true;
    for (int k = 0; k < ndir; ++k)
      ok = ok && (!dirs[k].dgh_next || (al16(dirs[k].dgh_next, dirs[k].ld_dgn) && al16(dirs[k].w_hh_t, dirs[k].ld_wt)));
    if (ok) {
      switch (gru_chunk(H)) {
        case 512: return gru_launch_bwd_fast<512>(a, ndir, st);
        case 256: return gru_launch_bwd_fast<256>(a, ndir, st);
        case 128: return gru_launch_bwd_fast<128>(a, ndir, st);
        case 64: return gru_launch_bwd_fast<64>(a, ndir, st);
        default: return gru_launch_bwd_fast<32>(a, ndir, st);
      }
    }
  }
  dim3 grid((B + 63) / 64, (H + 63) / 64, ndir);
  if (dtype == VMMT_F32) {
    size_t sm = gemm_smem_elems<float, 64, 64, 32>() * sizeof(float);
    hipLaunchKernelGGL(gru_step_bwd_kernel<float>, grid, dim3(256), sm, st, a);
  } else {
    size_t sm = gemm_smem_elems<bf16_t, 64, 64, 32>() * sizeof(bf16_t);
    hipLaunchKernelGGL(gru_step_bwd_kernel<bf16_t>, grid, dim3(256), sm, st, a);
  }
  return check_launch();
}

// a whole recurrence in one host call: nsteps launches, step i described by dirs[i*ndir .. i*ndir+ndir)
extern "C" int vmmt_gru_chain_fwd(int dtype, int ndir, int nsteps, const vmmt_gru_dir_fwd* dirs, const int64_t* lens, int B,
                                  int H, void* stream) {
  return vmmt::chain_steps(ndir, nsteps, dirs, [&](const vmmt_gru_dir_fwd* d) { return vmmt_gru_step_fwd(dtype, ndir, d, lens, B, H, stream); });
}

extern "C" int vmmt_gru_chain_bwd(int dtype, int ndir, int nsteps, const vmmt_gru_dir_bwd* dirs, const int64_t* lens, int B,
                                  int H, int mode, void* stream) {
  return vmmt::chain_steps(ndir, nsteps, dirs, [&](const vmmt_gru_dir_bwd* d) { return vmmt_gru_step_bwd(dtype, ndir, d, lens, B, H, mode, stream); });
}
