// Microbenchmark: the four 3 x 3 cross blocks of pgs_setup (lm_dynamics.h),  X[r][s](own, K) = sum_i T_own,r[i] * B_K,s[i]  over the four lanes
// K of a quad, in two formulations, on one wavefront per CU (64 lanes, the step kernels' launch shape):
//   dpp   the present one: per owner K three quad broadcasts (v_mov_b32_dpp quad_perm:[K,K,K,K]) and five multiply-adds per component i
//         (pgs_cross_blocks<K>, copied here instruction for instruction)
//   mfma  v_mfma_f32_4x4x1_16B_f32: sixteen independent 4 x 4 blocks, one per quad, D[i][j] += A(lane i) * B(lane j), lane j receiving D[0..3][j]:
//         with A = B_K,s[i] and B = T_own,r[i] one instruction gives a lane its products against all four owners; 9 accumulators x 6 components
// (a) shader cycles (s_memtime) per evaluation of each, alone and embedded between 100 independent v_fma_f32, on a dependency chain from
//     one evaluation to the next as in a sub-step; the cost of the chain itself (form "none") is reported next to them
// (b) the two formulations bit for bit on random inputs, with zeros, values around 1e-30 and denormal inputs among them
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-mfma-vgpr-form tools/microbench/mfma_quad_blocks.hip -o /tmp/mfma_quad_blocks && timeout 120 /tmp/mfma_quad_blocks
// Prints one JSON document (profiles/r05_mfma_quad_blocks.json).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include "../../locomanipulationrl_amd/csrc/lm_math.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define NOUT 36      // per lane: [K][r][s]

// t[i][r]: this lane's three contact rows, b[i][s]: its three B vectors (component i = 0 .. 5)
template <int K>
LM_DEV void cross_dpp(const float t[6][3], const float b[6][3], float* out) {
  float a00 = 0.f; f2 a0t = sp2(0.f), c0 = sp2(0.f), c1 = sp2(0.f), c2 = sp2(0.f);
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const float k0 = quad_bcast<K>(b[i][0]); const f2 k12 = mk2(quad_bcast<K>(b[i][1]), quad_bcast<K>(b[i][2]));
    const float t0 = t[i][0]; const f2 t12 = mk2(t[i][1], t[i][2]);
    a00 = fmaf(t0, k0, a00); a0t = fma_(sp2(t0), k12, a0t);
    c0 = fma_(t12, sp2(k0), c0); c1 = fma_(t12, sp2(k12.x), c1); c2 = fma_(t12, sp2(k12.y), c2);
  }
  out[9 * K + 0] = a00; out[9 * K + 1] = a0t.x; out[9 * K + 2] = a0t.y;          // row 0: columns 0, 1, 2
  out[9 * K + 3] = c0.x; out[9 * K + 4] = c1.x; out[9 * K + 5] = c2.x;           // row 1
  out[9 * K + 6] = c0.y; out[9 * K + 7] = c1.y; out[9 * K + 8] = c2.y;           // row 2
}
LM_DEV void blocks_dpp(const float t[6][3], const float b[6][3], float* out) {
  cross_dpp<0>(t, b, out); cross_dpp<1>(t, b, out); cross_dpp<2>(t, b, out); cross_dpp<3>(t, b, out);
}
LM_DEV void blocks_mfma(const float t[6][3], const float b[6][3], float* out) {
  f32x4 acc[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int s = 0; s < 3; s++) acc[r][s] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int s = 0; s < 3; s++) acc[r][s] = __builtin_amdgcn_mfma_f32_4x4x1f32(b[i][s], t[i][r], acc[r][s], 0, 0, 0);
#pragma unroll
  for (int K = 0; K < 4; K++)
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int s = 0; s < 3; s++) out[9 * K + 3 * r + s] = acc[r][s][K];
}

// (b) both formulations on the same inputs
__global__ void __launch_bounds__(64) k_compare(const float* __restrict__ in, float* __restrict__ od, float* __restrict__ om) {
  const size_t lane = (size_t)blockIdx.x * 64 + threadIdx.x;
  float t[6][3], b[6][3];
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int c = 0; c < 3; c++) { t[i][c] = in[lane * 36 + 3 * i + c]; b[i][c] = in[lane * 36 + 18 + 3 * i + c]; }
  float a[NOUT], m[NOUT];
  blocks_dpp(t, b, a); blocks_mfma(t, b, m);
#pragma unroll
  for (int k = 0; k < NOUT; k++) { od[lane * NOUT + k] = a[k]; om[lane * NOUT + k] = m[k]; }
}

// (a) FORM 0: the dependency chain alone, 1: dpp, 2: mfma.  EMBED: 100 v_fma_f32 on 25 independent accumulators in the same block of code
template <int FORM, int EMBED>
__global__ void __launch_bounds__(64) k_time(const float* __restrict__ in, float* __restrict__ sink, unsigned long long* __restrict__ ticks, int iters) {
  const size_t lane = (size_t)blockIdx.x * 64 + threadIdx.x;
  float t0[6][3], b0[6][3];
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int c = 0; c < 3; c++) { t0[i][c] = in[lane * 36 + 3 * i + c]; b0[i][c] = in[lane * 36 + 18 + 3 * i + c]; }
  float e = 0.f, f[25];
#pragma unroll
  for (int k = 0; k < 25; k++) f[k] = 1.0f + 0.01f * k;
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  __builtin_amdgcn_sched_barrier(0);
  for (int it = 0; it < iters; it++) {
    float t[6][3], b[6][3], o[NOUT];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
      for (int c = 0; c < 3; c++) { t[i][c] = t0[i][c] + e; b[i][c] = b0[i][c] + e; }          // every input waits for the evaluation before
    if (FORM == 1) blocks_dpp(t, b, o);
    else if (FORM == 2) blocks_mfma(t, b, o);
    else {
#pragma unroll
      for (int k = 0; k < NOUT; k++) o[k] = k < 18 ? t[k / 3][k % 3] : b[(k - 18) / 3][k % 3];
    }
    if (EMBED) {
#pragma unroll
      for (int round = 0; round < 4; round++)
#pragma unroll
        for (int k = 0; k < 25; k++) f[k] = fmaf(f[k], 0.999f, 1.0e-3f);
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NOUT; k++) s += o[k];          // ... and every output is needed by the next
    e = s * 1.0e-30f;
  }
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  float s = e;
#pragma unroll
  for (int k = 0; k < 25; k++) s += f[k];
  sink[lane] = s;
  if (threadIdx.x == 0) { ticks[2 * blockIdx.x] = c1 - c0; ticks[2 * blockIdx.x + 1] = r1 - r0; }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

template <int FORM, int EMBED>
static int time_form(const float* in, float* sink, unsigned long long* ticks, int blocks, int iters, double* cyc, double* us) {
  std::vector<unsigned long long> h(2 * blocks);
  for (int rep = 0; rep < 2; rep++) {          // the second launch is the measured one (code and inputs warm)
    hipLaunchKernelGGL((k_time<FORM, EMBED>), dim3(blocks), dim3(64), 0, 0, in, sink, ticks, iters);
    CHECK(hipDeviceSynchronize());
  }
  CHECK(hipMemcpy(h.data(), ticks, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
  std::vector<double> a, b;
  for (int k = 0; k < blocks; k++) { a.push_back((double)h[2 * k] / iters); b.push_back((double)h[2 * k + 1] / iters / 100.0); }      // s_memrealtime: 100 MHz
  *cyc = median(a); *us = median(b);
  return 0;
}

int main() {
  const int blocks = 256, lanes = blocks * 64, iters = 512;
  std::vector<float> h((size_t)lanes * 36);
  srand(5);
  auto u = [] { return (float)rand() / (float)RAND_MAX * 2.f - 1.f; };
  for (int l = 0; l < lanes; l++)
    for (int k = 0; k < 36; k++) {
      float v = u() * (k < 18 ? 1.0f : 10.0f);
      const int kind = (l / 64) % 8;          // per wavefront: 0-3 plain, 4 zeros among the entries, 5 around 1e-30, 6 denormal inputs, 7 a mix per lane
      const int sel = kind == 7 ? 4 + (l + k) % 4 : kind;
      if (sel == 4 && (rand() & 3) == 0) v = (rand() & 1) ? 0.f : -0.f;
      if (sel == 5) v *= 1.0e-30f;
      if (sel == 6 && (rand() & 1)) v *= 1.0e-40f;
      h[(size_t)l * 36 + k] = v;
    }
  float *in, *od, *om, *sink; unsigned long long* ticks;
  CHECK(hipMalloc(&in, h.size() * 4)); CHECK(hipMalloc(&od, (size_t)lanes * NOUT * 4)); CHECK(hipMalloc(&om, (size_t)lanes * NOUT * 4));
  CHECK(hipMalloc(&sink, (size_t)lanes * 4)); CHECK(hipMalloc(&ticks, (size_t)blocks * 2 * 8));
  CHECK(hipMemcpy(in, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  // (b)
  hipLaunchKernelGGL(k_compare, dim3(blocks), dim3(64), 0, 0, in, od, om);
  CHECK(hipDeviceSynchronize());
  std::vector<float> a((size_t)lanes * NOUT), m((size_t)lanes * NOUT);
  CHECK(hipMemcpy(a.data(), od, a.size() * 4, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(m.data(), om, m.size() * 4, hipMemcpyDeviceToHost));
  long diff[8] = {0}, total[8] = {0}, sign_of_zero[8] = {0}; double worst_rel[8] = {0};
  for (size_t k = 0; k < a.size(); k++) {
    const int kind = (int)((k / NOUT / 64) % 8);
    total[kind]++;
    if (memcmp(&a[k], &m[k], 4) != 0) {
      if (a[k] == m[k]) sign_of_zero[kind]++;          // +0 against -0
      else { diff[kind]++; const double rel = fabs((double)a[k] - (double)m[k]) / fmax(fabs((double)a[k]), 1e-300); if (rel > worst_rel[kind]) worst_rel[kind] = rel; }
    }
  }
  // (a)
  double cyc[3][2], us[3][2];
  if (time_form<0, 0>(in, sink, ticks, blocks, iters, &cyc[0][0], &us[0][0]) || time_form<1, 0>(in, sink, ticks, blocks, iters, &cyc[1][0], &us[1][0]) ||
      time_form<2, 0>(in, sink, ticks, blocks, iters, &cyc[2][0], &us[2][0]) || time_form<0, 1>(in, sink, ticks, blocks, iters, &cyc[0][1], &us[0][1]) ||
      time_form<1, 1>(in, sink, ticks, blocks, iters, &cyc[1][1], &us[1][1]) || time_form<2, 1>(in, sink, ticks, blocks, iters, &cyc[2][1], &us[2][1])) return 1;
  const char* kinds[8] = {"plain", "plain", "plain", "plain", "zeros among the entries", "scaled by 1e-30", "half the entries scaled by 1e-40 (denormal)", "mixed per lane"};
  printf("{\n \"what\": \"tools/microbench/mfma_quad_blocks.hip: the four 3x3 cross blocks of pgs_setup, DPP + FMA against 54 v_mfma_f32_4x4x1, one wavefront per CU, %d blocks x %d evaluations\",\n", blocks, iters);
  printf(" \"a_timing\": {\"unit\": \"per evaluation, median over the wavefronts: s_memtime ticks and microseconds (s_memrealtime)\",\n");
  const char* forms[3] = {"none", "dpp", "mfma"};
  for (int e = 0; e < 2; e++)
    for (int f = 0; f < 3; f++)
      printf("  \"%s_%s\": {\"memtime_ticks\": %.1f, \"us\": %.4f, \"ticks_minus_chain\": %.1f, \"us_minus_chain\": %.4f}%s\n", forms[f], e ? "embedded_in_100_fma" : "alone", cyc[f][e], us[f][e],
             cyc[f][e] - cyc[0][e], us[f][e] - us[0][e], (e == 1 && f == 2) ? "" : ",");
  printf(" },\n \"b_bit_identity\": {\"values_per_class\": \"36 per lane\",\n");
  for (int k = 0; k < 8; k++)
    printf("  \"wavefront_class_%d (%s)\": {\"values\": %ld, \"different_bits\": %ld, \"only_sign_of_zero\": %ld, \"worst_relative_difference\": %.3g}%s\n", k, kinds[k], total[k], diff[k], sign_of_zero[k], worst_rel[k], k == 7 ? "" : ",");
  printf(" }\n}\n");
  return 0;
}
