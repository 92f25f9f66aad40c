// lm_gnn_ppo.hip -- lm_gnn_ppo_grad (include/lm_policy.h): the loss and parameter gradient of one PPO mini-batch of train/ppo.py PPO.update for
// the GraphPolicy (policies/graph_model.py: input layers 16 -> 32 / 4 -> 32, three GraphLayers over the fixed 13-node, 24-edge tree with max
// aggregation, mean head on nodes 1..12, value head on the max over the nodes, log_std 12).  The semantics are those of lm_mlp_ppo_grad
// (csrc/lm_ppo.hip) with the network swapped; the operand maps of v_mfma_f32_16x16x4_f32 are the ones documented there.
//
// k_gnn_ppo_grad: persistent workgroups of 8 wavefronts (one per compute unit: 150 KB of LDS), each looping over sample tiles of 16.  A 16-column
// block of a matrix product is ONE node (or edge) x the tile's 16 samples, so all graph indexing is wave-uniform.  On-chip state of a tile:
//   three node buffers [13 nodes][16 samples][32] (row stride 36) and two edge buffers [12 edges][16][32]; nothing of it in global memory.
//   forward   h0 -> A, h1 -> B, h2 -> C, h3 -> A; one wave per target node: P = Wa h[t] once, then per incoming edge Q = Wb h[src],
//             hid = elu(P + Q + b1), m = elu(W2 hid + b2), out = max m - all in registers (an accumulator tile IS the next product's B operand)
//   loss      one lane per sample, in double (the MLP kernel's code); the 13 head dot products per sample on the vector ALU in double
//   backward  per layer, in two groups of 12 edges (targets 0..4, targets 5..12) so that the edge buffers fit:
//     R   per target node: recompute hid_e, m_e, the max and the number of edges that attain it; d pre2_e = d out / ties * [m_e == max] * elu'
//     W2  dW2 += d pre2^T hid  (K = the 192 edge rows), db2
//     R2  d pre1_e = (W2^T d pre2_e) * elu'(hid_e), in place
//     W1  dW1 += [d pre1^T h[tgt] | d pre1^T h[src]], db1;  d h[v] (+)= Wa^T sum_{e into v} d pre1_e + Wb^T sum_{e out of v} d pre1_e
//   The layer inputs are not all kept: h3 overwrites h0, and h0 (from the observations) and h1 are recomputed when their layer's backward
//   needs them (one extra layer forward per tile) - that is what lets the tile fit the LDS with no stash in the workspace.
// Every dot product of the forward goes in runs of 16 into two fresh fp32 accumulators (8 terms each) that are added in double, as ppo_fwd does.
// Determinism: no atomics; per-workgroup partial sums in the workspace, added in a fixed order in double by k_gnn_ppo_reduce.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lm_policy.h"
#include "../../include/lm_engine.h"
#include "lm_internal.h"

typedef float gnn_f4 __attribute__((ext_vector_type(4)));
#define GNN_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

#define GNN_TILE 16            // samples per tile
#define GNN_THREADS 512        // 8 wavefronts
#define GNN_NW 8
#define GNN_MAX_GROUPS 1024
#define GNN_SN 36              // row stride of the node / edge buffers (32 features + 4: float4 rows stay 16-byte aligned)
#define GNN_SO 68              // row stride of the observation tile
#define GNN_NODE_ROWS (13 * GNN_TILE)
#define GNN_EDGE_ROWS (12 * GNN_TILE)

// flat parameter block (torch layout, the order include/lm_policy.h fixes)
enum {
  GNN_oWi1 = 0, GNN_obi1 = 512, GNN_oWi2 = 544, GNN_obi2 = 672, GNN_oL = 704, GNN_LS = 3136,      // a GraphLayer: W1 (32,64) b1 W2 (32,32) b2
  GNN_W1 = 0, GNN_b1 = 2048, GNN_W2 = 2080, GNN_b2 = 3104,
  GNN_oWm = GNN_oL + 3 * GNN_LS, GNN_obm = GNN_oWm + 32, GNN_oWv = GNN_obm + 1, GNN_obv = GNN_oWv + 32, GNN_ols = GNN_obv + 1, GNN_P = GNN_ols + 12,
  GNN_PS = (GNN_P + 3 + 3) / 4 * 4      // workspace row: P gradients + 3 loss sums, padded to 4
};
static_assert(GNN_P == 10190, "the flat GNN block of include/lm_policy.h");

struct __attribute__((aligned(16))) GnnSmem {
  float A[GNN_NODE_ROWS * GNN_SN], B[GNN_NODE_ROWS * GNN_SN], C[GNN_NODE_ROWS * GNN_SN];
  float EA[GNN_EDGE_ROWS * GNN_SN], EB[GNN_EDGE_ROWS * GNN_SN];
  float xo[GNN_TILE * GNN_SO];      // the tile's observations
  double hv[GNN_TILE * 16];         // per sample: 12 means and the value, as the heads' double sums give them
  float hd[GNN_TILE * 16];          // per sample: the deltas of the 12 means and of the value
  float gls[GNN_TILE * 12];         // per sample: d loss / d log_std_j (policy part)
  float st[GNN_TILE * 4];           // per sample: -surrogate, (ret - v_clipped)^2, kl term
  double ls[12], istd[12];          // log_std and exp(-log_std), once per launch
};

struct GnnArgs {
  const float *params, *obs, *act, *old_logp, *old_val, *adv, *ret;
  float* ws; int B, ntiles;
  double r_lo, r_hi; float vclip, vscale;
};

__device__ __forceinline__ float gnn_elu(float z) { return z > 0.f ? z : expm1f(z); }
__device__ __forceinline__ float gnn_delu(float y) { return y > 0.f ? 1.f : y + 1.f; }      // ELU' from the ELU's OUTPUT y

// the tree: node 0 the object, joints 1..4 under it, 5..8 under those, 9..12 under those; every tree edge in both directions
__device__ __forceinline__ int gnn_deg(int t) { return t == 0 ? 4 : (t < 9 ? 2 : 1); }
__device__ __forceinline__ int gnn_src(int t, int q) {      // source of the q-th edge into t
  if (t == 0) return 1 + q;
  if (t < 5) return q == 0 ? 0 : t + 4;
  if (t < 9) return q == 0 ? t - 4 : t + 4;
  return t - 4;
}
// the two edge groups of the backward: group 0 = the 12 edges into nodes 0..4, group 1 = the 12 edges into nodes 5..12; slot = place in the group
__device__ __forceinline__ int gnn_slot(int t, int q) { return t == 0 ? q : (t < 5 ? 4 + 2 * (t - 1) + q : (t < 9 ? 2 * (t - 5) + q : 8 + (t - 9))); }
__device__ __forceinline__ int gnn_slot_tgt(int grp, int s) { return grp == 0 ? (s < 4 ? 0 : 1 + ((s - 4) >> 1)) : (s < 8 ? 5 + (s >> 1) : 9 + (s - 8)); }
__device__ __forceinline__ int gnn_slot_q(int grp, int s) { return grp == 0 ? (s < 4 ? s : ((s - 4) & 1)) : (s < 8 ? (s & 1) : 0); }
// column of joint k (0..11) inside each 12-wide group of the observation (create_features)
__device__ __forceinline__ int gnn_jcol(int k) { return k < 4 ? k : (k < 8 ? 4 + 2 * (k - 4) : 5 + 2 * (k - 8)); }

// the parameter pointer as a value the optimiser cannot trace: keeps the (loop-invariant) weight loads of one phase from being hoisted over the
// whole tile loop, where the three layers' weights together would not fit the register file
__device__ __forceinline__ const float* gnn_opaque(const float* p) { asm volatile("" : "+s"(p)); return p; }

// rows of one node / edge slot as a matrix operand: lane (n, g) holds features 16 a + 4 g + 0..3 of sample n
__device__ __forceinline__ void gnn_load(const float* H, int blk, gnn_f4 (&x)[2], int lane) {
  const int n = lane & 15, g = lane >> 4;
#pragma unroll
  for (int a = 0; a < 2; a++) x[a] = *reinterpret_cast<const gnn_f4*>(&H[(blk * GNN_TILE + n) * GNN_SN + a * 16 + 4 * g]);
}
__device__ __forceinline__ void gnn_store(float* H, int blk, const gnn_f4 (&x)[2], int lane) {
  const int n = lane & 15, g = lane >> 4;
#pragma unroll
  for (int a = 0; a < 2; a++) *reinterpret_cast<gnn_f4*>(&H[(blk * GNN_TILE + n) * GNN_SN + a * 16 + 4 * g]) = x[a];
}

// sum[a][r] += sum_{k < 32} W[(16 a + n') ld + k] x[k] for output feature 16 a + 4 g + r, sample n: each run of 16 k values goes into two fresh
// accumulators (8 terms each) that are added in double
__device__ __forceinline__ void gnn_mm(const float* __restrict__ W, int ld, const gnn_f4 (&x)[2], double (&sum)[2][4], int lane) {
  const int n = lane & 15, g = lane >> 4;
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int kc = 0; kc < 2; kc++) {
      const gnn_f4 wv = *reinterpret_cast<const gnn_f4*>(&W[(a * 16 + n) * ld + kc * 16 + 4 * g]);
      gnn_f4 acc[2] = {gnn_f4{0.f, 0.f, 0.f, 0.f}, gnn_f4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j & 1] = GNN_MFMA(wv[j], x[kc][j], acc[j & 1]);
#pragma unroll
      for (int r = 0; r < 4; r++) sum[a][r] += (double)acc[0][r] + (double)acc[1][r];
    }
}

// acc[c][r] += sum_{o < 32} W[o ld + 16 c + 4 g + r] d[o]  (the transposed product of the backward; plain fp32 accumulation)
__device__ __forceinline__ void gnn_mmT(const float* __restrict__ W, int ld, const gnn_f4 (&d)[2], gnn_f4 (&acc)[2], int lane) {
  const int n = lane & 15, g = lane >> 4;
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int o = a * 16 + 4 * g + j;
#pragma unroll
      for (int c = 0; c < 2; c++) acc[c] = GNN_MFMA(W[o * ld + c * 16 + n], d[a][j], acc[c]);
    }
}

// one edge: hid = elu(P + Wb h_src + b1), m = elu(W2 hid + b2); L = the layer's parameters
__device__ __forceinline__ void gnn_edge(const float* __restrict__ L, const double (&Pd)[2][4], const gnn_f4 (&xs)[2], gnn_f4 (&hid)[2], gnn_f4 (&m)[2], int lane) {
  const int g = lane >> 4;
  double S[2][4], Z[2][4];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) { S[a][r] = Pd[a][r]; Z[a][r] = 0.0; }
  gnn_mm(L + GNN_W1 + 32, 64, xs, S, lane);
#pragma unroll
  for (int a = 0; a < 2; a++) {
    const gnn_f4 bv = *reinterpret_cast<const gnn_f4*>(&L[GNN_b1 + a * 16 + 4 * g]);
#pragma unroll
    for (int r = 0; r < 4; r++) hid[a][r] = gnn_elu((float)(S[a][r] + (double)bv[r]));
  }
  gnn_mm(L + GNN_W2, 32, hid, Z, lane);
#pragma unroll
  for (int a = 0; a < 2; a++) {
    const gnn_f4 bv = *reinterpret_cast<const gnn_f4*>(&L[GNN_b2 + a * 16 + 4 * g]);
#pragma unroll
    for (int r = 0; r < 4; r++) m[a][r] = gnn_elu((float)(Z[a][r] + (double)bv[r]));
  }
}

// h0: node 0 = input_layer1(obs[0:16]), node k = input_layer2(the four columns of joint k - 1); no activation
__device__ __forceinline__ void gnn_input_fwd(const float* Pp, const float* xo, float* H, int w, int lane) {
  const float* __restrict__ P = gnn_opaque(Pp);
  const int n = lane & 15, g = lane >> 4;
#pragma unroll 1
  for (int t = w; t < 13; t += GNN_NW) {
    gnn_f4 y[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
      gnn_f4 acc[2] = {gnn_f4{0.f, 0.f, 0.f, 0.f}, gnn_f4{0.f, 0.f, 0.f, 0.f}};
      gnn_f4 bv;
      if (t == 0) {
        const gnn_f4 wv = *reinterpret_cast<const gnn_f4*>(&P[GNN_oWi1 + (a * 16 + n) * 16 + 4 * g]);
        const gnn_f4 xv = *reinterpret_cast<const gnn_f4*>(&xo[n * GNN_SO + 4 * g]);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j & 1] = GNN_MFMA(wv[j], xv[j], acc[j & 1]);
        bv = *reinterpret_cast<const gnn_f4*>(&P[GNN_obi1 + a * 16 + 4 * g]);
      } else {
        acc[0] = GNN_MFMA(P[GNN_oWi2 + (a * 16 + n) * 4 + g], xo[n * GNN_SO + 16 + 12 * g + gnn_jcol(t - 1)], acc[0]);
        bv = *reinterpret_cast<const gnn_f4*>(&P[GNN_obi2 + a * 16 + 4 * g]);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) y[a][r] = (float)((double)acc[0][r] + (double)acc[1][r] + (double)bv[r]);
    }
    gnn_store(H, t, y, lane);
  }
}

// one GraphLayer forward: Hout[t] = max over the edges into t, one wave per target node
__device__ __forceinline__ void gnn_layer_fwd(const float* Lp, const float* Hin, float* Hout, int w, int lane) {
  const float* __restrict__ L = gnn_opaque(Lp);
#pragma unroll 1
  for (int t = w; t < 13; t += GNN_NW) {
    gnn_f4 xt[2]; gnn_load(Hin, t, xt, lane);
    double Pd[2][4];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int r = 0; r < 4; r++) Pd[a][r] = 0.0;
    gnn_mm(L + GNN_W1, 64, xt, Pd, lane);
    const gnn_f4 ninf4 = gnn_f4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    gnn_f4 mx[2] = {ninf4, ninf4};
    const int deg = gnn_deg(t);
#pragma unroll 1
    for (int q = 0; q < deg; q++) {
      gnn_f4 xs[2], hid[2], m[2];
      gnn_load(Hin, gnn_src(t, q), xs, lane);
      gnn_edge(L, Pd, xs, hid, m, lane);
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int r = 0; r < 4; r++) mx[a][r] = fmaxf(mx[a][r], m[a][r]);
    }
    gnn_store(Hout, t, mx, lane);
  }
}

// one GraphLayer backward.  Hin = the layer's input, DO = d loss / d output, DH <- d loss / d input; accW1 / accW2 = this wave's blocks of
// dW1 (wave w: rows 16 (w & 1), columns 32 ((w >> 1) & 1) + 16 (w >> 2)) and dW2 (waves 0..3: rows 16 (w & 1), columns 16 (w >> 1));
// csum = this thread's column sum when it owns b1[tid - cb1] or b2[tid - cb1 - 32] of this layer.  Ends on a barrier.
__device__ __forceinline__ void gnn_layer_bwd(const float* Lp, const float* Hin, const float* DO, float* DH, float* EA, float* EB,
                                              gnn_f4& accW1, gnn_f4& accW2, double& csum, int cb1, int tid, int w) {
  const int lane = tid & 63, n = lane & 15, g = lane >> 4;
#pragma unroll 1
  for (int grp = 0; grp < 2; grp++) {
    const int t0 = grp ? 5 : 0, nt = grp ? 8 : 5;
    const float* L = gnn_opaque(Lp);
    // ---- R: hid_e -> EB, d pre2_e -> EA for the edges into this wave's target nodes
#pragma unroll 1
    for (int ti = w; ti < nt; ti += GNN_NW) {
      const int t = t0 + ti, deg = gnn_deg(t);
      gnn_f4 xt[2]; gnn_load(Hin, t, xt, lane);
      double Pd[2][4];
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int r = 0; r < 4; r++) Pd[a][r] = 0.0;
      gnn_mm(L + GNN_W1, 64, xt, Pd, lane);
      const gnn_f4 ninf4 = gnn_f4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      gnn_f4 mx[2] = {ninf4, ninf4};
#pragma unroll 1
      for (int q = 0; q < deg; q++) {
        gnn_f4 xs[2], hid[2], m[2];
        gnn_load(Hin, gnn_src(t, q), xs, lane);
        gnn_edge(L, Pd, xs, hid, m, lane);
        gnn_store(EB, gnn_slot(t, q), hid, lane); gnn_store(EA, gnn_slot(t, q), m, lane);      // (m is read back by this lane only: no barrier)
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
          for (int r = 0; r < 4; r++) mx[a][r] = fmaxf(mx[a][r], m[a][r]);
      }
      gnn_f4 share[2]; gnn_load(DO, t, share, lane);
      if (deg > 1) {      // exact ties split the gradient evenly (autograd's amax)
        gnn_f4 cnt[2] = {gnn_f4{0.f, 0.f, 0.f, 0.f}, gnn_f4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 1
        for (int q = 0; q < deg; q++) {
          gnn_f4 m[2]; gnn_load(EA, gnn_slot(t, q), m, lane);
#pragma unroll
          for (int a = 0; a < 2; a++)
#pragma unroll
            for (int r = 0; r < 4; r++) cnt[a][r] += m[a][r] == mx[a][r] ? 1.f : 0.f;
        }
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
          for (int r = 0; r < 4; r++) share[a][r] = cnt[a][r] == 1.f ? share[a][r] : share[a][r] / cnt[a][r];
      }
#pragma unroll 1
      for (int q = 0; q < deg; q++) {
        gnn_f4 m[2]; gnn_load(EA, gnn_slot(t, q), m, lane);
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
          for (int r = 0; r < 4; r++) m[a][r] = m[a][r] == mx[a][r] ? share[a][r] * gnn_delu(m[a][r]) : 0.f;
        gnn_store(EA, gnn_slot(t, q), m, lane);
      }
    }
    __syncthreads();
    // ---- W2: dW2 += d pre2^T hid over the group's 192 edge rows; db2
    if (w < 4) {
      const int o = 16 * (w & 1) + n, i = 16 * (w >> 1) + n;
#pragma unroll 4
      for (int q = 0; q < GNN_EDGE_ROWS / 4; q++) {
        const int row = 4 * q + g;
        accW2 = GNN_MFMA(EA[row * GNN_SN + o], EB[row * GNN_SN + i], accW2);
      }
    }
    if (tid >= cb1 + 32 && tid < cb1 + 64) {
      const int o = tid - cb1 - 32;
#pragma unroll 8
      for (int row = 0; row < GNN_EDGE_ROWS; row++) csum += (double)EA[row * GNN_SN + o];
    }
    __syncthreads();
    L = gnn_opaque(Lp);
    // ---- R2: d pre1_e = (W2^T d pre2_e) * elu'(hid_e), in place (a lane rewrites the words it read)
#pragma unroll 1
    for (int slot = w; slot < 12; slot += GNN_NW) {
      gnn_f4 d[2], hid[2], acc[2] = {gnn_f4{0.f, 0.f, 0.f, 0.f}, gnn_f4{0.f, 0.f, 0.f, 0.f}};
      gnn_load(EA, slot, d, lane); gnn_load(EB, slot, hid, lane);
      gnn_mmT(L + GNN_W2, 32, d, acc, lane);
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[a][r] *= gnn_delu(hid[a][r]);
      gnn_store(EA, slot, acc, lane);
    }
    __syncthreads();
    // ---- W1: dW1 += [d pre1^T h[tgt] | d pre1^T h[src]]; db1; d h
    {
      const int o = 16 * (w & 1) + n, half = (w >> 1) & 1, i = 16 * (w >> 2) + n;
#pragma unroll 1
      for (int slot = 0; slot < 12; slot++) {
        const int tgt = gnn_slot_tgt(grp, slot), node = half ? gnn_src(tgt, gnn_slot_q(grp, slot)) : tgt;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int s = 4 * q + g;
          accW1 = GNN_MFMA(EA[(slot * GNN_TILE + s) * GNN_SN + o], Hin[(node * GNN_TILE + s) * GNN_SN + i], accW1);
        }
      }
    }
    if (tid >= cb1 && tid < cb1 + 32) {
      const int o = tid - cb1;
#pragma unroll 8
      for (int row = 0; row < GNN_EDGE_ROWS; row++) csum += (double)EA[row * GNN_SN + o];
    }
    L = gnn_opaque(Lp);
#pragma unroll 1
    for (int v = w; v < 13; v += GNN_NW) {
      gnn_f4 dP[2] = {gnn_f4{0.f, 0.f, 0.f, 0.f}, gnn_f4{0.f, 0.f, 0.f, 0.f}}, dQ[2] = {gnn_f4{0.f, 0.f, 0.f, 0.f}, gnn_f4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 1
      for (int slot = 0; slot < 12; slot++) {
        const int tgt = gnn_slot_tgt(grp, slot), src = gnn_src(tgt, gnn_slot_q(grp, slot));
        if (tgt == v || src == v) {
          gnn_f4 d[2]; gnn_load(EA, slot, d, lane);
#pragma unroll
          for (int a = 0; a < 2; a++) { if (tgt == v) dP[a] += d[a]; else dQ[a] += d[a]; }
        }
      }
      gnn_f4 acc[2] = {gnn_f4{0.f, 0.f, 0.f, 0.f}, gnn_f4{0.f, 0.f, 0.f, 0.f}};
      gnn_mmT(L + GNN_W1, 64, dP, acc, lane);
      gnn_mmT(L + GNN_W1 + 32, 64, dQ, acc, lane);
      if (grp) {      // the same lane wrote these words in group 0
        gnn_f4 old[2]; gnn_load(DH, v, old, lane);
#pragma unroll
        for (int a = 0; a < 2; a++) acc[a] += old[a];
      }
      gnn_store(DH, v, acc, lane);
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(GNN_THREADS) k_gnn_ppo_grad(GnnArgs A) {
  __shared__ GnnSmem M;
  const int tid0 = threadIdx.x;
  const float* __restrict__ P = A.params;
  const gnn_f4 zero4 = gnn_f4{0.f, 0.f, 0.f, 0.f};
  // this wave's gradient blocks, in registers over the tiles: dW1 and dW2 of the three layers, and a block of an input layer (waves 4..7)
  gnn_f4 aW1_0 = zero4, aW1_1 = zero4, aW1_2 = zero4, aW2_0 = zero4, aW2_1 = zero4, aW2_2 = zero4, aIn = zero4;
  // column sums (bias gradients, the head gradients, log_std, the loss sums): one per thread, in double
  //   tid 0..31 bi1 | 32..63 bi2 | 64 + 64 l + (0..31) b1 of layer l | 96 + 64 l + (0..31) b2 of layer l | 256..287 Wm | 288..319 Wv | 320 bm | 321 bv |
  //   322..333 log_std | 334..336 the loss sums
  int cout = -1;
  {
  const int tid = tid0;
  if (tid < 32) cout = GNN_obi1 + tid;
  else if (tid < 64) cout = GNN_obi2 + tid - 32;
  else if (tid < 256) { const int l = (tid - 64) >> 6, c = (tid - 64) & 63; cout = GNN_oL + l * GNN_LS + (c < 32 ? GNN_b1 + c : GNN_b2 + c - 32); }
  else if (tid < 288) cout = GNN_oWm + tid - 256;
  else if (tid < 320) cout = GNN_oWv + tid - 288;
  else if (tid == 320) cout = GNN_obm;
  else if (tid == 321) cout = GNN_obv;
  else if (tid < 334) cout = GNN_ols + tid - 322;
  else if (tid < 337) cout = GNN_P + tid - 334;
  }
  double csum = 0.0;

  if (tid0 < 12) { const int tid = tid0; const double l = (double)P[GNN_ols + tid]; M.ls[tid] = l; M.istd[tid] = exp(-l); }      // (the tile loop's first barrier orders it)

  for (int tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
    const int b0 = tile * GNN_TILE;
    // the thread index as a value of this iteration: the tile's hundreds of (loop-invariant) LDS addresses are then computed where they are
    // used instead of being hoisted over the tile loop and spilled
    int tid = tid0; asm volatile("" : "+v"(tid));
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), n = lane & 15, g = lane >> 4;
    // ---- the tile's observations (rows past B are zeros)
    for (int idx = tid; idx < GNN_TILE * 16; idx += GNN_THREADS) {
      const int s = idx >> 4, k = (idx & 15) * 4;
      gnn_f4 v = zero4;
      if (b0 + s < A.B) v = *reinterpret_cast<const gnn_f4*>(&A.obs[(size_t)(b0 + s) * 64 + k]);
      *reinterpret_cast<gnn_f4*>(&M.xo[s * GNN_SO + k]) = v;
    }
    __syncthreads();
    // ---- forward: h0 -> A, h1 -> B, h2 -> C, h3 -> A
    gnn_input_fwd(P, M.xo, M.A, w, lane);
    __syncthreads();
    gnn_layer_fwd(P + GNN_oL, M.A, M.B, w, lane);
    __syncthreads();
    gnn_layer_fwd(P + GNN_oL + GNN_LS, M.B, M.C, w, lane);
    __syncthreads();
    gnn_layer_fwd(P + GNN_oL + 2 * GNN_LS, M.C, M.A, w, lane);
    __syncthreads();
    // ---- heads, in double on the vector ALU: thread (node, sample); node 0 computes the value from the max over the nodes
    if (tid < GNN_NODE_ROWS) {
      const int s = tid & 15, node = tid >> 4;
      double acc = 0.0;
      if (node == 0) {
#pragma unroll 1
        for (int f = 0; f < 32; f++) {
          float mxv = M.A[s * GNN_SN + f];
#pragma unroll 1
          for (int v = 1; v < 13; v++) mxv = fmaxf(mxv, M.A[(v * GNN_TILE + s) * GNN_SN + f]);
          acc += (double)P[GNN_oWv + f] * (double)mxv;
        }
        M.hv[s * 16 + 12] = acc + (double)P[GNN_obv];
      } else {
#pragma unroll 1
        for (int f = 0; f < 32; f++) acc += (double)P[GNN_oWm + f] * (double)M.A[(node * GNN_TILE + s) * GNN_SN + f];
        M.hv[s * 16 + node - 1] = acc + (double)P[GNN_obm];
      }
    }
    __syncthreads();
    // ---- loss: one lane per sample (k_ppo_grad's code, on the heads' double outputs); hd receives the head deltas
    if (tid < GNN_TILE) {
      const int s = tid, b = b0 + s;
      float* h = &M.hd[s * 16];
      const double* hv = &M.hv[s * 16];
      if (b < A.B) {
        double lp = 0.0;
#pragma unroll
        for (int j = 0; j < 12; j++) {
          const double z = ((double)A.act[(size_t)b * 12 + j] - hv[j]) * M.istd[j];
          lp += -0.5 * (z * z) - M.ls[j] - 0.91893853320467274178;
        }
        const double rl = lp - (double)A.old_logp[b], ratio = exp(rl), ad = (double)A.adv[b];
        const double rc = fmin(fmax(ratio, A.r_lo), A.r_hi), t1 = ad * ratio, t2 = ad * rc;
        const bool live = (rc == ratio) || (t1 < t2);
        const double glp = live ? -t1 : 0.0;
#pragma unroll
        for (int j = 0; j < 12; j++) {
          const double z = ((double)A.act[(size_t)b * 12 + j] - hv[j]) * M.istd[j];
          h[j] = (float)(glp * (z * M.istd[j]));
          M.gls[s * 12 + j] = (float)(glp * (z * z - 1.0));
        }
        const double ov = (double)A.old_val[b], dv = hv[12] - ov, vcl = (double)A.vclip;
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
    }
    __syncthreads();
    // ---- backward through the heads: d h3 -> B, thread (sample, feature).  The value head's gradient goes to the maximal node, the lowest
    // index on an exact tie
    {
      const int s = tid >> 5, f = tid & 31;
      int arg = 0; float mxv = M.A[s * GNN_SN + f];
#pragma unroll 1
      for (int v = 1; v < 13; v++) { const float x = M.A[(v * GNN_TILE + s) * GNN_SN + f]; if (x > mxv) { mxv = x; arg = v; } }
      const float wm = P[GNN_oWm + f], dval = M.hd[s * 16 + 12] * P[GNN_oWv + f];
#pragma unroll 1
      for (int v = 0; v < 13; v++) {
        float d = v ? M.hd[s * 16 + v - 1] * wm : 0.f;
        if (v == arg) d += dval;
        M.B[(v * GNN_TILE + s) * GNN_SN + f] = d;
      }
    }
    if (tid >= 256 && tid < 288) {      // d Wm[f] = sum_{s, k} d mean[s][k] h3[k + 1][s][f]
      const int f = tid - 256;
#pragma unroll 1
      for (int v = 1; v < 13; v++)
#pragma unroll 1
        for (int s = 0; s < GNN_TILE; s++) csum += (double)M.hd[s * 16 + v - 1] * (double)M.A[(v * GNN_TILE + s) * GNN_SN + f];
    } else if (tid >= 288 && tid < 320) {      // d Wv[f] = sum_s d v[s] max_v h3[v][s][f]
      const int f = tid - 288;
#pragma unroll 1
      for (int s = 0; s < GNN_TILE; s++) {
        float mxv = M.A[s * GNN_SN + f];
#pragma unroll 1
        for (int v = 1; v < 13; v++) mxv = fmaxf(mxv, M.A[(v * GNN_TILE + s) * GNN_SN + f]);
        csum += (double)M.hd[s * 16 + 12] * (double)mxv;
      }
    } else if (tid == 320) {
#pragma unroll 1
      for (int s = 0; s < GNN_TILE; s++)
#pragma unroll 1
        for (int k = 0; k < 12; k++) csum += (double)M.hd[s * 16 + k];
    } else if (tid == 321) {
#pragma unroll 1
      for (int s = 0; s < GNN_TILE; s++) csum += (double)M.hd[s * 16 + 12];
    } else if (tid >= 322 && tid < 334) {
#pragma unroll 1
      for (int s = 0; s < GNN_TILE; s++) csum += (double)M.gls[s * 12 + tid - 322];
    } else if (tid >= 334 && tid < 337) {
#pragma unroll 1
      for (int s = 0; s < GNN_TILE; s++) csum += (double)M.st[s * 4 + tid - 334];
    }
    __syncthreads();
    // ---- backward through the layers (each call ends on a barrier)
    gnn_layer_bwd(P + GNN_oL + 2 * GNN_LS, M.C, M.B, M.A, M.EA, M.EB, aW1_2, aW2_2, csum, 64 + 128, tid, w);      // h2 in C, d h3 in B -> d h2 in A
    gnn_input_fwd(P, M.xo, M.B, w, lane);                                                                     // h0 -> B
    __syncthreads();
    gnn_layer_fwd(P + GNN_oL, M.B, M.C, w, lane);                                                             // h1 -> C
    __syncthreads();
    gnn_layer_bwd(P + GNN_oL + GNN_LS, M.C, M.A, M.B, M.EA, M.EB, aW1_1, aW2_1, csum, 64 + 64, tid, w);          // d h2 in A -> d h1 in B
    gnn_input_fwd(P, M.xo, M.A, w, lane);                                                                     // h0 -> A
    __syncthreads();
    gnn_layer_bwd(P + GNN_oL, M.A, M.B, M.C, M.EA, M.EB, aW1_0, aW2_0, csum, 64, tid, w);                        // d h1 in B -> d h0 in C
    // ---- the input layers: d Wi1 = d h0[0]^T obs[:, 0:16] (waves 4, 5), d Wi2 = sum over the joints d h0[k]^T joint_k (waves 6, 7), biases
    if (w >= 4 && w < 6) {
      const int o = 16 * (w - 4) + n;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int s = 4 * q + g;
        aIn = GNN_MFMA(M.C[s * GNN_SN + o], M.xo[s * GNN_SO + n], aIn);
      }
    } else if (w >= 6) {
      const int o = 16 * (w - 6) + n;
#pragma unroll 1
      for (int v = 1; v < 13; v++) {
        const int col = 16 + 12 * (n & 3) + gnn_jcol(v - 1);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int s = 4 * q + g;
          aIn = GNN_MFMA(M.C[(v * GNN_TILE + s) * GNN_SN + o], n < 4 ? M.xo[s * GNN_SO + col] : 0.f, aIn);
        }
      }
    }
    if (tid < 32) {
#pragma unroll 1
      for (int s = 0; s < GNN_TILE; s++) csum += (double)M.C[s * GNN_SN + tid];
    } else if (tid < 64) {
#pragma unroll 8
      for (int row = GNN_TILE; row < GNN_NODE_ROWS; row++) csum += (double)M.C[row * GNN_SN + tid - 32];
    }
    __syncthreads();
  }

  // ---- this workgroup's partial sums: every slot of its workspace row that the reduction reads is written, whatever was there
  float* __restrict__ out = A.ws + (size_t)blockIdx.x * GNN_PS;
  {
    const int lane = tid0 & 63, w = tid0 >> 6, n = lane & 15, g = lane >> 4;
    const int o = 16 * (w & 1) + 4 * g, i1 = 32 * ((w >> 1) & 1) + 16 * (w >> 2) + n, i2 = 16 * (w >> 1) + n;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      out[GNN_oL + GNN_W1 + (o + r) * 64 + i1] = aW1_0[r];
      out[GNN_oL + GNN_LS + GNN_W1 + (o + r) * 64 + i1] = aW1_1[r];
      out[GNN_oL + 2 * GNN_LS + GNN_W1 + (o + r) * 64 + i1] = aW1_2[r];
      if (w < 4) {
        out[GNN_oL + GNN_W2 + (o + r) * 32 + i2] = aW2_0[r];
        out[GNN_oL + GNN_LS + GNN_W2 + (o + r) * 32 + i2] = aW2_1[r];
        out[GNN_oL + 2 * GNN_LS + GNN_W2 + (o + r) * 32 + i2] = aW2_2[r];
      } else if (w < 6) {
        out[GNN_oWi1 + (16 * (w - 4) + 4 * g + r) * 16 + n] = aIn[r];
      } else if (n < 4) {
        out[GNN_oWi2 + (16 * (w - 6) + 4 * g + r) * 4 + n] = aIn[r];
      }
    }
  }
  if (cout >= 0) out[cout] = (float)csum;
}

// grad[p] = (sum over the workgroups' rows, fixed order) / B, the entropy term on log_std; stats = loss_pi, loss_v, kl, entropy
__global__ void __launch_bounds__(256) k_gnn_ppo_reduce(const float* __restrict__ ws, int groups, int B, float vscale, float escale,
                                                        const float* __restrict__ params, float* __restrict__ grad, float* __restrict__ stats) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx > GNN_P + 3) return;
  if (idx == GNN_P + 3) {
    float e = 0.f;
    for (int j = 0; j < 12; j++) e += params[GNN_ols + j] + 0.5f + 0.9189385332046727f;
    stats[3] = e;
    return;
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int gidx = 0;
  for (; gidx + 3 < groups; gidx += 4) {
    s0 += ws[(size_t)gidx * GNN_PS + idx]; s1 += ws[(size_t)(gidx + 1) * GNN_PS + idx];
    s2 += ws[(size_t)(gidx + 2) * GNN_PS + idx]; s3 += ws[(size_t)(gidx + 3) * GNN_PS + idx];
  }
  if (gidx < groups) s0 += ws[(size_t)gidx * GNN_PS + idx];
  if (gidx + 1 < groups) s1 += ws[(size_t)(gidx + 1) * GNN_PS + idx];
  if (gidx + 2 < groups) s2 += ws[(size_t)(gidx + 2) * GNN_PS + idx];
  const float m = (float)(((s0 + s1) + (s2 + s3)) / (double)B);
  if (idx < GNN_P) grad[idx] = idx >= GNN_ols ? m - escale : m;
  else if (idx == GNN_P) stats[0] = m;
  else if (idx == GNN_P + 1) stats[1] = vscale * m;
  else stats[2] = m;
}

static int gnn_groups_max() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) return -1;
  return cus < GNN_MAX_GROUPS ? cus : GNN_MAX_GROUPS;
}

static int gnn_on_current_device(const void* p) {
  hipPointerAttribute_t at; int dev = -1;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  return at.type == hipMemoryTypeDevice && at.device == dev;
}

extern "C" {

int lm_gnn_grad_param_count(void) { return GNN_P; }

int lm_gnn_ppo_grad_geometry(int B, int* tile, int* groups) {
  if (B < 1 || !tile || !groups) return lm_internal_fail(LM_EINVAL, "lm_gnn_ppo_grad_geometry: B >= 1 and both outputs non-null are needed");
  const int gmax = gnn_groups_max();
  if (gmax < 1) return lm_internal_fail(-2, "lm_gnn_ppo_grad_geometry: no HIP device to size the launch for");
  const int ntiles = (int)(((long long)B + GNN_TILE - 1) / GNN_TILE);
  *tile = GNN_TILE; *groups = ntiles < gmax ? ntiles : gmax;
  return 0;
}

long long lm_gnn_ppo_grad_workspace(int B) {
  int tile = 0, groups = 0;
  const int rc = lm_gnn_ppo_grad_geometry(B, &tile, &groups);
  if (rc) return rc;
  return (long long)groups * GNN_PS * (long long)sizeof(float);
}

int lm_gnn_ppo_grad(const float* params, const float* obs_n, const float* actions, const float* old_logp, const float* old_value_n, const float* adv,
                    const float* ret_n, int B, const lm_ppo_hyper* hp, float* grad, float* stats, void* workspace, long long workspace_bytes,
                    void* stream) {
  if (!params || !obs_n || !actions || !old_logp || !old_value_n || !adv || !ret_n || !hp || !grad || !stats || !workspace)
    return lm_internal_fail(LM_EINVAL, "lm_gnn_ppo_grad: null argument");
  if (B < 1) return lm_internal_fail(LM_EINVAL, "lm_gnn_ppo_grad: B must be >= 1");
  if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(obs_n) | reinterpret_cast<uintptr_t>(workspace)) & 15)
    return lm_internal_fail(LM_EINVAL, "lm_gnn_ppo_grad: params, obs_n and the workspace must be 16-byte aligned (read with 16-byte loads)");
  if (!gnn_on_current_device(params) || !gnn_on_current_device(grad) || !gnn_on_current_device(workspace))
    return lm_internal_fail(LM_EINVAL, "lm_gnn_ppo_grad: the buffers are not device memory of the calling thread's current device");
  int tile = 0, groups = 0;
  const int rc = lm_gnn_ppo_grad_geometry(B, &tile, &groups);
  if (rc) return rc;
  if (workspace_bytes < (long long)groups * GNN_PS * (long long)sizeof(float)) return lm_internal_fail(LM_EINVAL, "lm_gnn_ppo_grad: the workspace is smaller than lm_gnn_ppo_grad_workspace(B)");
  GnnArgs A;
  A.params = params; A.obs = obs_n; A.act = actions; A.old_logp = old_logp; A.old_val = old_value_n; A.adv = adv; A.ret = ret_n;
  A.ws = (float*)workspace; A.B = B; A.ntiles = (int)(((long long)B + GNN_TILE - 1) / GNN_TILE);
  A.r_lo = 1.0 - (double)hp->ratio_clip; A.r_hi = 1.0 + (double)hp->ratio_clip; A.vclip = hp->value_clip; A.vscale = hp->value_scale;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gnn_ppo_grad, dim3(groups), dim3(GNN_THREADS), 0, s, A);
  if (hipGetLastError() != hipSuccess) return lm_internal_fail(-2, "lm_gnn_ppo_grad: launching the gradient kernel failed");
  hipLaunchKernelGGL(k_gnn_ppo_reduce, dim3((GNN_P + 4 + 255) / 256), dim3(256), 0, s, (const float*)workspace, groups, B, hp->value_scale, hp->entropy_scale,
                     params, grad, stats);
  return hipGetLastError() == hipSuccess ? 0 : lm_internal_fail(-2, "lm_gnn_ppo_grad: launching the reduction failed");
}

}  // extern "C"
