// lm_ppo.hip -- the PPO update's two device pieces (include/lm_policy.h): lm_mlp_ppo_grad, the loss and parameter gradient of one mini-batch
// of train/ppo.py PPO.update for the SharedMLP (64/88-256-128-64, ELU, mean head 12, value head 1, log_std 12), and lm_gae.
//
// k_ppo_grad: persistent workgroups of 8 wavefronts (at most one per compute unit: ~147 KB of LDS), each looping over sample tiles of 32.
// Per tile, with every activation and every delta of the tile in LDS as fp32 [sample][feature] and nothing of it in global memory:
//   forward   Z(out x samples) = W(out x K) X(K x samples)      A operand = the weights, read from the flat torch-layout block (L2) as float4
//   loss      one lane per sample, in double: logp, ratio, both clips, the head deltas (without the 1/B factor: applied once, in the reduction)
//   backward  D(in x samples)  = W^T(in x out) Dn(out x samples), times ELU'(a) = (a > 0 ? 1 : a + 1)
//   dW(out x in) += Dl(out x samples) A(samples x in)           all 58 649 (88-wide: 64 793) accumulators stay in registers over the tiles
// Every product is v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation (== an fmaf chain), so the kernel's error is that of an
// fp32 summation order, and small deltas need no scaling (there is no fp16 half that could go subnormal).  The forward shortens its chains to
// 8 terms and adds them in double (ppo_fwd); the per-sample loss and every sum over samples outside the matrix pipe are in double as well.
// Operand maps (16x16x4, lane l, n = l & 15, g = l >> 4): A[m = n][k = g], B[k = g][col = n], D[row = 4 g + r][col = n] in register r.
// A run of 16 k values is covered by 4 instructions with lane group g taking k = 4 g + j in instruction j: both operands then come from ONE
// float4 per lane (the order of the k terms inside a dot product is permuted, the same way for both operands).
// Determinism: no atomics.  A workgroup writes its partial gradient (and three loss sums) to its own row of the workspace; k_ppo_reduce adds
// the rows in a fixed order (four interleaved chains in double, then (s0 + s1) + (s2 + s3)), divides by B and applies the entropy term.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lm_policy.h"
#include "../../include/lm_engine.h"
#include "lm_internal.h"

typedef float ppo_f4 __attribute__((ext_vector_type(4)));
#define PPO_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

#define PPO_TILE 32            // samples per tile
#define PPO_THREADS 512        // 8 wavefronts
#define PPO_MAX_GROUPS 1024

// flat parameter block (torch layout, the order include/lm_policy.h fixes) and the LDS row strides (all = 20 mod 32 words: the float4 reads of
// 8 consecutive samples and the 16-lane dword runs of the dW operands both spread over the banks)
template <int NOBS> struct PpoLayout {
  static constexpr int K0 = (NOBS + 15) / 16 * 16;                  // 64 | 96: the observation padded with zeros in LDS
  static constexpr int oW1 = 0, ob1 = 256 * NOBS, oW2 = ob1 + 256, ob2 = oW2 + 128 * 256, oW3 = ob2 + 128, ob3 = oW3 + 64 * 128;
  static constexpr int oWm = ob3 + 64, obm = oWm + 12 * 64, oWv = obm + 12, obv = oWv + 64, ols = obv + 1, P = ols + 12;
  static constexpr int PS = (P + 3 + 3) / 4 * 4;                     // workspace row: P gradients + 3 loss sums, padded to 4
  static constexpr int S0 = K0 + 20, S1 = 276, S2 = 148, S3 = 84, SH = 20;
};

template <int NOBS> struct PpoSmem {
  typedef PpoLayout<NOBS> L;
  float x0[PPO_TILE * L::S0], a1[PPO_TILE * L::S1], a2[PPO_TILE * L::S2], a3[PPO_TILE * L::S3];
  float d1[PPO_TILE * L::S1], d2[PPO_TILE * L::S2], d3[PPO_TILE * L::S3], dh[PPO_TILE * L::SH];
  float gls[PPO_TILE * 12];      // per sample: d loss / d log_std_j (policy part)
  float st[PPO_TILE * 4];        // per sample: -surrogate, (ret - v_clipped)^2, kl term
  double ls[12], istd[12];       // log_std and exp(-log_std), once per launch
};

struct PpoArgs {
  const float *params, *obs, *act, *old_logp, *old_val, *adv, *ret;
  float* ws; int B, ntiles;
  double r_lo, r_hi; float vclip, vscale;
};

__device__ __forceinline__ float ppo_elu(float z) { return z > 0.f ? z : expm1f(z); }

// one trunk layer forward for NOB output blocks x NSB sample blocks of this wave; KV = the weight rows' real length (K padded beyond it).
// A dot product is NOT one fp32 chain over K: each run of 16 k values goes into two fresh accumulators (8 terms each) and the runs are added
// in double on the vector ALU (2 x 4 conversions and adds per tile and run, next to 4 matrix instructions).  One fp32 chain over K = 256 terms
// loses about sqrt(K) half-ulps of the running sum; this loses about the final rounding.  The difference shows in kl = (ratio - 1) - rl,
// which cancels to O(rl^2) and so magnifies the error of the means.
template <int K, int KV, int SX, int SY, int NOB, int NSB>
__device__ __forceinline__ void ppo_fwd(const float* __restrict__ W, const float* __restrict__ bias, const float* X, float* Y, int ob0, int sb0, int lane) {
  const int n = lane & 15, g = lane >> 4;
  double sum[NOB][NSB][4];
#pragma unroll
  for (int a = 0; a < NOB; a++)
#pragma unroll
    for (int b = 0; b < NSB; b++)
#pragma unroll
      for (int r = 0; r < 4; r++) sum[a][b][r] = 0.0;
#pragma unroll 2
  for (int kc = 0; kc < K / 16; kc++) {
    const int k = kc * 16 + 4 * g;
    ppo_f4 xb[NSB];
#pragma unroll
    for (int b = 0; b < NSB; b++) xb[b] = *reinterpret_cast<const ppo_f4*>(&X[((sb0 + b) * 16 + n) * SX + k]);
#pragma unroll
    for (int a = 0; a < NOB; a++) {
      const int row = (ob0 + a) * 16 + n;
      ppo_f4 w = ppo_f4{0.f, 0.f, 0.f, 0.f};
      if (KV == K || k < KV) w = *reinterpret_cast<const ppo_f4*>(&W[(size_t)row * KV + k]);
      ppo_f4 acc[NSB][2];
#pragma unroll
      for (int b = 0; b < NSB; b++) { acc[b][0] = ppo_f4{0.f, 0.f, 0.f, 0.f}; acc[b][1] = ppo_f4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int b = 0; b < NSB; b++) acc[b][j & 1] = PPO_MFMA(w[j], xb[b][j], acc[b][j & 1]);
#pragma unroll
      for (int b = 0; b < NSB; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) sum[a][b][r] += (double)acc[b][0][r] + (double)acc[b][1][r];
    }
  }
#pragma unroll
  for (int a = 0; a < NOB; a++) {
    const int o = (ob0 + a) * 16 + 4 * g;
    const ppo_f4 bv = *reinterpret_cast<const ppo_f4*>(&bias[o]);
#pragma unroll
    for (int b = 0; b < NSB; b++) {
      ppo_f4 y;
#pragma unroll
      for (int r = 0; r < 4; r++) y[r] = ppo_elu((float)(sum[a][b][r] + (double)bv[r]));
      *reinterpret_cast<ppo_f4*>(&Y[((sb0 + b) * 16 + n) * SY + o]) = y;
    }
  }
}

// deltas of a trunk layer: Dout[s][i] = (sum_o W[o][i] Dn[s][o]) * ELU'(A[s][i]) for NIB input blocks x NSB sample blocks of this wave
template <int KO, int NI, int SD, int SA, int NIB, int NSB>
__device__ __forceinline__ void ppo_bwd(const float* __restrict__ W, const float* Dn, const float* A, float* Dout, int ib0, int sb0, int lane) {
  const int n = lane & 15, g = lane >> 4;
  ppo_f4 acc[NIB][NSB];
#pragma unroll
  for (int a = 0; a < NIB; a++)
#pragma unroll
    for (int b = 0; b < NSB; b++) acc[a][b] = ppo_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int oc = 0; oc < KO / 16; oc++) {
    const int o = oc * 16 + 4 * g;
    ppo_f4 db[NSB];
#pragma unroll
    for (int b = 0; b < NSB; b++) db[b] = *reinterpret_cast<const ppo_f4*>(&Dn[((sb0 + b) * 16 + n) * SD + o]);
#pragma unroll
    for (int a = 0; a < NIB; a++) {
      const int i = (ib0 + a) * 16 + n;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float w = W[(size_t)(o + j) * NI + i];
#pragma unroll
        for (int b = 0; b < NSB; b++) acc[a][b] = PPO_MFMA(w, db[b][j], acc[a][b]);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NIB; a++) {
    const int i = (ib0 + a) * 16 + 4 * g;
#pragma unroll
    for (int b = 0; b < NSB; b++) {
      const int s = (sb0 + b) * 16 + n;
      const ppo_f4 av = *reinterpret_cast<const ppo_f4*>(&A[s * SA + i]);
      ppo_f4 y;
#pragma unroll
      for (int r = 0; r < 4; r++) y[r] = acc[a][b][r] * (av[r] > 0.f ? 1.f : av[r] + 1.f);
      *reinterpret_cast<ppo_f4*>(&Dout[s * SA + i]) = y;
    }
  }
}

// dW[o0 + ..16][i0 + 16 cb + ..16] += sum over the tile's 32 samples of Dl[s][o] Ap[s][i]
template <int NCB, int SD, int SA>
__device__ __forceinline__ void ppo_dw(ppo_f4 (&acc)[NCB], const float* Dl, const float* Ap, int o0, int i0, int lane) {
  const int n = lane & 15, g = lane >> 4;
#pragma unroll 2
  for (int q = 0; q < PPO_TILE / 4; q++) {
    const int s = 4 * q + g;
    const float a = Dl[s * SD + o0 + n];
#pragma unroll
    for (int cb = 0; cb < NCB; cb++) acc[cb] = PPO_MFMA(a, Ap[s * SA + i0 + 16 * cb + n], acc[cb]);
  }
}

template <int NCB>
__device__ __forceinline__ void ppo_dw_store(const ppo_f4 (&acc)[NCB], float* __restrict__ out, int ld, int o0, int i0, int ncols, int lane) {
  const int n = lane & 15, g = lane >> 4;
#pragma unroll
  for (int cb = 0; cb < NCB; cb++) {
    const int i = i0 + 16 * cb + n;
    if (i < ncols) {
#pragma unroll
      for (int r = 0; r < 4; r++) out[(size_t)(o0 + 4 * g + r) * ld + i] = acc[cb][r];
    }
  }
}

template <int NOBS>
__global__ void __launch_bounds__(PPO_THREADS) k_ppo_grad(PpoArgs A) {
  typedef PpoLayout<NOBS> L;
  __shared__ PpoSmem<NOBS> M;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g = lane >> 4;
  const float* __restrict__ P = A.params;
  constexpr int NCB1 = L::K0 / 16;
  ppo_f4 acc1[2][NCB1], acc2[16], acc3[4], acch[1];
  const ppo_f4 zero4 = ppo_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < NCB1; b++) acc1[a][b] = zero4;
#pragma unroll
  for (int b = 0; b < 16; b++) acc2[b] = zero4;
#pragma unroll
  for (int b = 0; b < 4; b++) acc3[b] = zero4;
  acch[0] = zero4;

  // column sums (bias gradients, log_std gradient, loss sums): one column of one LDS array per thread, summed over the samples in order
  const float* col = nullptr; int cstride = 0, cout = -1;
  if (tid < 256) { col = &M.d1[tid]; cstride = L::S1; cout = L::ob1 + tid; }
  else if (tid < 384) { col = &M.d2[tid - 256]; cstride = L::S2; cout = L::ob2 + tid - 256; }
  else if (tid < 448) { col = &M.d3[tid - 384]; cstride = L::S3; cout = L::ob3 + tid - 384; }
  else if (tid < 461) { col = &M.dh[tid - 448]; cstride = L::SH; cout = tid < 460 ? L::obm + tid - 448 : L::obv; }
  else if (tid < 473) { col = &M.gls[tid - 461]; cstride = 12; cout = L::ols + tid - 461; }
  else if (tid < 476) { col = &M.st[tid - 473]; cstride = 4; cout = L::P + tid - 473; }
  double csum = 0.0;      // 32 adds per tile: double costs nothing here and takes the summation order out of the bias gradients and loss sums

  if (tid < 12) { const double l = (double)P[L::ols + tid]; M.ls[tid] = l; M.istd[tid] = exp(-l); }      // (the tile loop's first barrier orders it)

  for (int tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    const int b0 = tile * PPO_TILE;
    // ---- the tile's observations (rows past B and columns past NOBS are zeros)
    for (int idx = tid; idx < PPO_TILE * (L::K0 / 4); idx += PPO_THREADS) {
      const int s = idx / (L::K0 / 4), k = (idx % (L::K0 / 4)) * 4;
      ppo_f4 v = zero4;
      if (b0 + s < A.B && k < NOBS) v = *reinterpret_cast<const ppo_f4*>(&A.obs[(size_t)(b0 + s) * NOBS + k]);
      *reinterpret_cast<ppo_f4*>(&M.x0[s * L::S0 + k]) = v;
    }
    __syncthreads();
    // ---- forward
    ppo_fwd<L::K0, NOBS, L::S0, L::S1, 2, 2>(P + L::oW1, P + L::ob1, M.x0, M.a1, 2 * w, 0, lane);
    __syncthreads();
    ppo_fwd<256, 256, L::S1, L::S2, 1, 2>(P + L::oW2, P + L::ob2, M.a1, M.a2, w, 0, lane);
    __syncthreads();
    ppo_fwd<128, 128, L::S2, L::S3, 1, 1>(P + L::oW3, P + L::ob3, M.a2, M.a3, w & 3, w >> 2, lane);
    __syncthreads();
    if (w < 2) {      // heads: rows 0..11 the mean layer, row 12 the value layer, rows 13..15 zero
      const float* wrow = n < 12 ? P + L::oWm + n * 64 : P + L::oWv;
      double sum[4] = {0.0, 0.0, 0.0, 0.0};      // runs of 16 added in double, as in ppo_fwd
#pragma unroll
      for (int kc = 0; kc < 4; kc++) {
        ppo_f4 acc[2] = {zero4, zero4};
        const int k = kc * 16 + 4 * g;
        const ppo_f4 xb = *reinterpret_cast<const ppo_f4*>(&M.a3[(w * 16 + n) * L::S3 + k]);
        ppo_f4 wv = zero4;
        if (n < 13) wv = *reinterpret_cast<const ppo_f4*>(&wrow[k]);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j & 1] = PPO_MFMA(wv[j], xb[j], acc[j & 1]);
#pragma unroll
        for (int r = 0; r < 4; r++) sum[r] += (double)acc[0][r] + (double)acc[1][r];
      }
      ppo_f4 y;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int o = 4 * g + r;
        y[r] = (float)(sum[r] + (double)(o < 12 ? P[L::obm + o] : (o == 12 ? P[L::obv] : 0.f)));
      }
      *reinterpret_cast<ppo_f4*>(&M.dh[(w * 16 + n) * L::SH + 4 * g]) = y;
    }
    __syncthreads();
    // ---- loss: one lane per sample; the head outputs in dh become the head deltas
    if (tid < PPO_TILE) {
      const int s = tid, b = b0 + s;
      float* h = &M.dh[s * L::SH];
      if (b < A.B) {
        // in double: one lane per sample, so it costs next to nothing, and the sum of twelve O(1) terms to a log-probability of O(10) is
        // where fp32 loses the ratio's last digits (kl = (ratio - 1) - rl cancels to O(rl^2))
        double lp = 0.0;
#pragma unroll
        for (int j = 0; j < 12; j++) {
          const double z = ((double)A.act[(size_t)b * 12 + j] - (double)h[j]) * M.istd[j];
          lp += -0.5 * (z * z) - M.ls[j] - 0.91893853320467274178;
        }
        const double rl = lp - (double)A.old_logp[b], ratio = exp(rl), ad = (double)A.adv[b];
        const double rc = fmin(fmax(ratio, A.r_lo), A.r_hi), t1 = ad * ratio, t2 = ad * rc;
        const bool live = (rc == ratio) || (t1 < t2);
        const double glp = live ? -t1 : 0.0;
#pragma unroll
        for (int j = 0; j < 12; j++) {      // z again rather than twelve doubles kept over the exp
          const double z = ((double)A.act[(size_t)b * 12 + j] - (double)h[j]) * M.istd[j];
          h[j] = (float)(glp * (z * M.istd[j]));
          M.gls[s * 12 + j] = (float)(glp * (z * z - 1.0));
        }
        const double ov = (double)A.old_val[b], dv = (double)h[12] - ov, vcl = (double)A.vclip;
        const double dvc = fmin(fmax(dv, -vcl), vcl), e = (double)A.ret[b] - (ov + dvc);
        h[12] = (dvc == dv) ? (float)(-2.0 * (double)A.vscale * e) : 0.f;
        M.st[s * 4 + 0] = (float)(-fmin(t1, t2)); M.st[s * 4 + 1] = (float)(e * e); M.st[s * 4 + 2] = (float)((ratio - 1.0) - rl);
      } else {
#pragma unroll
        for (int j = 0; j < 13; j++) h[j] = 0.f;
#pragma unroll
        for (int j = 0; j < 12; j++) M.gls[s * 12 + j] = 0.f;
        M.st[s * 4 + 0] = 0.f; M.st[s * 4 + 1] = 0.f; M.st[s * 4 + 2] = 0.f;
      }
      h[13] = 0.f; h[14] = 0.f; h[15] = 0.f;
    }
    __syncthreads();
    // ---- backward through the heads, head weight gradients
    {
      const int ib = w & 3, sb = w >> 2, i = ib * 16 + n;
      const ppo_f4 db = *reinterpret_cast<const ppo_f4*>(&M.dh[(sb * 16 + n) * L::SH + 4 * g]);
      ppo_f4 acc = zero4;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int o = 4 * g + j;
        const float wv = o < 12 ? P[L::oWm + o * 64 + i] : (o == 12 ? P[L::oWv + i] : 0.f);
        acc = PPO_MFMA(wv, db[j], acc);
      }
      const int s = sb * 16 + n, i4 = ib * 16 + 4 * g;
      const ppo_f4 av = *reinterpret_cast<const ppo_f4*>(&M.a3[s * L::S3 + i4]);
      ppo_f4 y;
#pragma unroll
      for (int r = 0; r < 4; r++) y[r] = acc[r] * (av[r] > 0.f ? 1.f : av[r] + 1.f);
      *reinterpret_cast<ppo_f4*>(&M.d3[s * L::S3 + i4]) = y;
      if (w < 4) ppo_dw<1, L::SH, L::S3>(acch, M.dh, M.a3, 0, 16 * w, lane);
    }
    __syncthreads();
    ppo_bwd<64, 128, L::S3, L::S2, 1, 2>(P + L::oW3, M.d3, M.a2, M.d2, w, 0, lane);
    ppo_dw<4, L::S3, L::S2>(acc3, M.d3, M.a2, 16 * (w & 3), 64 * (w >> 2), lane);
    __syncthreads();
    ppo_bwd<128, 256, L::S2, L::S1, 2, 2>(P + L::oW2, M.d2, M.a1, M.d1, 2 * w, 0, lane);
    ppo_dw<16, L::S2, L::S1>(acc2, M.d2, M.a1, 16 * w, 0, lane);
    __syncthreads();
    ppo_dw<NCB1, L::S1, L::S0>(acc1[0], M.d1, M.x0, 32 * w, 0, lane);
    ppo_dw<NCB1, L::S1, L::S0>(acc1[1], M.d1, M.x0, 32 * w + 16, 0, lane);
    if (col) {
#pragma unroll 8
      for (int s = 0; s < PPO_TILE; s++) csum += (double)col[s * cstride];
    }
    __syncthreads();
  }

  // ---- this workgroup's partial sums: every slot of its workspace row that the reduction reads is written, whatever was there
  float* __restrict__ out = A.ws + (size_t)blockIdx.x * L::PS;
  ppo_dw_store<NCB1>(acc1[0], out + L::oW1, NOBS, 32 * w, 0, NOBS, lane);
  ppo_dw_store<NCB1>(acc1[1], out + L::oW1, NOBS, 32 * w + 16, 0, NOBS, lane);
  ppo_dw_store<16>(acc2, out + L::oW2, 256, 16 * w, 0, 256, lane);
  ppo_dw_store<4>(acc3, out + L::oW3, 128, 16 * (w & 3), 64 * (w >> 2), 128, lane);
  if (w < 4) {
    const int i = 16 * w + n;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int o = 4 * g + r;
      if (o < 12) out[L::oWm + o * 64 + i] = acch[0][r];
      else if (o == 12) out[L::oWv + i] = acch[0][r];
    }
  }
  if (cout >= 0) out[cout] = (float)csum;
}

// grad[p] = (sum over the workgroups' rows, fixed order) / B, the entropy term on log_std; stats = loss_pi, loss_v, kl, entropy
__global__ void __launch_bounds__(256) k_ppo_reduce(const float* __restrict__ ws, int groups, int PS, int P, int ols, int B, float vscale, float escale,
                                                    const float* __restrict__ params, float* __restrict__ grad, float* __restrict__ stats) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx > P + 3) return;
  if (idx == P + 3) {
    float e = 0.f;
    for (int j = 0; j < 12; j++) e += params[ols + j] + 0.5f + 0.9189385332046727f;
    stats[3] = e;
    return;
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;      // memory-bound: the double adds are free
  int gidx = 0;
  for (; gidx + 3 < groups; gidx += 4) {
    s0 += ws[(size_t)gidx * PS + idx]; s1 += ws[(size_t)(gidx + 1) * PS + idx];
    s2 += ws[(size_t)(gidx + 2) * PS + idx]; s3 += ws[(size_t)(gidx + 3) * PS + idx];
  }
  if (gidx < groups) s0 += ws[(size_t)gidx * PS + idx];
  if (gidx + 1 < groups) s1 += ws[(size_t)(gidx + 1) * PS + idx];
  if (gidx + 2 < groups) s2 += ws[(size_t)(gidx + 2) * PS + idx];
  const float m = (float)(((s0 + s1) + (s2 + s3)) / (double)B);
  if (idx < P) grad[idx] = idx >= ols ? m - escale : m;
  else if (idx == P) stats[0] = m;
  else if (idx == P + 1) stats[1] = vscale * m;
  else stats[2] = m;
}

// GAE(gamma, lambda): one lane per env walks t = T-1 .. 0; every operation rounded once, in the order of distributed.compute_gae
__global__ void __launch_bounds__(256) k_gae(const float* __restrict__ rew, const float* __restrict__ val, const int64_t* __restrict__ done,
                                             const float* __restrict__ last_value, int T, int N, float g32, float gl32,
                                             float* __restrict__ ret, float* __restrict__ adv) {
#pragma clang fp contract(off)      // every operator below rounds once: no v_fma / v_fmac (the __f*_rn intrinsics would not do: they are inline functions
                                    // compiled under the default contraction mode, and the compiler fuses them after inlining)
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  float nxt = last_value[e], last = 0.f;
  for (int t = T - 1; t >= 0; t--) {
    const size_t i = (size_t)t * N + e;
    const float v = val[i];
    const float nd = 1.0f - (float)done[i];
    const float delta = (rew[i] + (g32 * nxt) * nd) - v;
    last = delta + (gl32 * nd) * last;
    adv[i] = last; ret[i] = last + v;
    nxt = v;
  }
}

static int ppo_groups_max() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) return -1;
  return cus < PPO_MAX_GROUPS ? cus : PPO_MAX_GROUPS;
}

static int ppo_on_current_device(const void* p) {
  hipPointerAttribute_t at; int dev = -1;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  return at.type == hipMemoryTypeDevice && at.device == dev;
}

extern "C" {

int lm_mlp_grad_param_count(int num_obs) { return num_obs == 64 ? PpoLayout<64>::P : (num_obs == 88 ? PpoLayout<88>::P : -1); }

int lm_mlp_ppo_grad_geometry(int num_obs, int B, int* tile, int* groups) {
  if ((num_obs != 64 && num_obs != 88) || B < 1 || !tile || !groups) return lm_internal_fail(LM_EINVAL, "lm_mlp_ppo_grad_geometry: num_obs must be 64 or 88, B >= 1, and both outputs non-null");
  const int gmax = ppo_groups_max();
  if (gmax < 1) return lm_internal_fail(-2, "lm_mlp_ppo_grad_geometry: no HIP device to size the launch for");
  const int ntiles = (int)(((long long)B + PPO_TILE - 1) / PPO_TILE);
  *tile = PPO_TILE; *groups = ntiles < gmax ? ntiles : gmax;
  return 0;
}

long long lm_mlp_ppo_grad_workspace(int num_obs, int B) {
  int tile = 0, groups = 0;
  const int rc = lm_mlp_ppo_grad_geometry(num_obs, B, &tile, &groups);
  if (rc) return rc;
  return (long long)groups * (num_obs == 64 ? PpoLayout<64>::PS : PpoLayout<88>::PS) * (long long)sizeof(float);
}

int lm_mlp_ppo_grad(const float* params, const float* obs_n, const float* actions, const float* old_logp, const float* old_value_n, const float* adv,
                    const float* ret_n, int B, int num_obs, const lm_ppo_hyper* hp, float* grad, float* stats, void* workspace,
                    long long workspace_bytes, void* stream) {
  if (!params || !obs_n || !actions || !old_logp || !old_value_n || !adv || !ret_n || !hp || !grad || !stats || !workspace)
    return lm_internal_fail(LM_EINVAL, "lm_mlp_ppo_grad: null argument");
  if (B < 1 || (num_obs != 64 && num_obs != 88)) return lm_internal_fail(LM_EINVAL, "lm_mlp_ppo_grad: B must be >= 1 and num_obs 64 or 88");
  if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(obs_n) | reinterpret_cast<uintptr_t>(workspace)) & 15)
    return lm_internal_fail(LM_EINVAL, "lm_mlp_ppo_grad: params, obs_n and the workspace must be 16-byte aligned (read with 16-byte loads)");
  if (!ppo_on_current_device(params) || !ppo_on_current_device(grad) || !ppo_on_current_device(workspace))
    return lm_internal_fail(LM_EINVAL, "lm_mlp_ppo_grad: the buffers are not device memory of the calling thread's current device");
  int tile = 0, groups = 0;
  const int rc = lm_mlp_ppo_grad_geometry(num_obs, B, &tile, &groups);
  if (rc) return rc;
  const int PS = num_obs == 64 ? PpoLayout<64>::PS : PpoLayout<88>::PS, P = lm_mlp_grad_param_count(num_obs);
  if (workspace_bytes < (long long)groups * PS * (long long)sizeof(float)) return lm_internal_fail(LM_EINVAL, "lm_mlp_ppo_grad: the workspace is smaller than lm_mlp_ppo_grad_workspace(num_obs, B)");
  PpoArgs A;
  A.params = params; A.obs = obs_n; A.act = actions; A.old_logp = old_logp; A.old_val = old_value_n; A.adv = adv; A.ret = ret_n;
  A.ws = (float*)workspace; A.B = B; A.ntiles = (int)(((long long)B + PPO_TILE - 1) / PPO_TILE);
  A.r_lo = 1.0 - (double)hp->ratio_clip; A.r_hi = 1.0 + (double)hp->ratio_clip; A.vclip = hp->value_clip; A.vscale = hp->value_scale;
  hipStream_t s = (hipStream_t)stream;
  if (num_obs == 64) hipLaunchKernelGGL(k_ppo_grad<64>, dim3(groups), dim3(PPO_THREADS), 0, s, A);
  else hipLaunchKernelGGL(k_ppo_grad<88>, dim3(groups), dim3(PPO_THREADS), 0, s, A);
  if (hipGetLastError() != hipSuccess) return lm_internal_fail(-2, "lm_mlp_ppo_grad: launching the gradient kernel failed");
  const int ols = num_obs == 64 ? PpoLayout<64>::ols : PpoLayout<88>::ols;
  hipLaunchKernelGGL(k_ppo_reduce, dim3((P + 4 + 255) / 256), dim3(256), 0, s, (const float*)workspace, groups, PS, P, ols, B, hp->value_scale, hp->entropy_scale,
                     params, grad, stats);
  return hipGetLastError() == hipSuccess ? 0 : lm_internal_fail(-2, "lm_mlp_ppo_grad: launching the reduction failed");
}

int lm_gae(const float* rewards, const float* values, const int64_t* dones, const float* last_value, int T, int N, double gamma, double lam,
           float* returns, float* advantages, void* stream) {
  if (!rewards || !values || !dones || !last_value || !returns || !advantages || T < 1 || N < 1) return lm_internal_fail(LM_EINVAL, "lm_gae: null argument, T < 1 or N < 1");
  hipLaunchKernelGGL(k_gae, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, rewards, values, dones, last_value, T, N, (float)gamma, (float)(gamma * lam),
                     returns, advantages);
  return hipGetLastError() == hipSuccess ? 0 : lm_internal_fail(-2, "lm_gae: launch failed");
}

}  // extern "C"
