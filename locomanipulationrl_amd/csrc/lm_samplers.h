// lm_samplers.h -- device code of the step, layer 1 of 4: hashes, sin/cos and the counter-based domain-randomisation samplers.
// The four layers (lm_samplers.h, lm_dynamics.h, lm_task.h, lm_step.h) are one declaration sequence cut at its seams: both translation units
// that hold step kernels (lm_engine.hip, lm_engine_w2.hip) include them in this order.
#pragma once
#include "lm_math.h"
#include "lm_rng.h"
#include "../../include/lm_engine.h"

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
LM_DEV uint32_t mix32(uint32_t x) { return lm_mix32(x); }
LM_DEV void hash_uniform3(uint32_t seed, uint32_t env, uint32_t episode, float* u) {
  uint32_t base = mix32(seed ^ mix32(env * 0x9E3779B9U + 0x7F4A7C15U) ^ mix32(episode * 0x85EBCA6BU + 0x165667B1U));
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) { uint32_t r = mix32(base + (k + 1U) * 0xC2B2AE35U); u[k] = (float)(r >> 8) * (1.0f / 16777216.0f); }
}
// sin/cos for |x| up to a few turns (joint angles are bounded by +-pi): Cody-Waite reduction to [-pi/4, pi/4] and
// the single-precision minimax polynomials of Cephes sinf/cosf; absolute error ~1e-7, ~25 instructions
// (the libm sincosf carries a large-argument Payne-Hanek path that costs ~150).
LM_DEV void lm_sincos(float x, float* s, float* c) {
  float kf = rintf(x * 0.636619772367581343f);          // 2/pi
  int k = (int)kf;
  float r = fmaf(-kf, 1.57079625129699707031f, x);       // pi/2 split in three parts
  r = fmaf(-kf, 7.54978941586159635335e-8f, r);
  r = fmaf(-kf, 5.39030285815811905290e-15f, r);
  float z = r * r;
  float sp = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), z * r, r);
  float cp = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), z * z, fmaf(-0.5f, z, 1.0f));
  float ss = (k & 1) ? cp : sp, cc = (k & 1) ? sp : cp;
  *s = (k & 2) ? -ss : ss;
  *c = ((k + 1) & 2) ? -cc : cc;
}

// ---- domain randomisation: counter-based samples, same bits as oracle lmo_dr_sample up to fp32 rounding of log / cos
LM_DEV float dr_sample(uint32_t seed, uint32_t stream, uint32_t env, uint32_t key, uint32_t idx, int dist, float p0, float p1) {
  // components 2p and 2p+1 share one pair of uniforms (Box-Muller's cosine and sine branches): calls for neighbouring components
  // share the hashes, the logarithm, the square root and the sincos after common-subexpression elimination
  const uint32_t pair = idx >> 1; const bool odd = (idx & 1U) != 0;
  float u1, u2; lm_rng_pair(lm_rng_base(seed, stream, env, key), pair, &u1, &u2);
  if (dist == LM_DR_GAUSSIAN) { float sn, cs; lm_sincos(6.283185307179586f * u2, &sn, &cs); return p0 + p1 * (sqrtf(-2.0f * logf(u1)) * (odd ? sn : cs)); }
  const float u = odd ? u1 - (1.0f / 16777216.0f) : u2;
  if (dist == LM_DR_UNIFORM) return p0 + (p1 - p0) * u;
  return expf(logf(p0) + (logf(p1) - logf(p0)) * u);
}
LM_DEV float dr_apply(int op, float x, float n) { return op == LM_DR_ADDITIVE ? x + n : (op == LM_DR_SCALING ? x * n : n); }
// one randomised physics attribute: on_interval entries are redrawn every `interval` control steps, on_reset entries at the env's
// last gated reset (reset_key 0 = never randomised)
LM_DEV float dr_attr(const lm_dr_channel& ch, uint32_t seed, uint32_t stream, int env, uint32_t dr_step, uint32_t reset_key, int idx, int comp, float base) {
  if (!ch.enabled) return base;
  uint32_t key = ch.interval > 0 ? dr_step / (uint32_t)ch.interval : reset_key;
  if (ch.interval == 0 && key == 0) return base;
  return dr_apply(ch.operation, base, dr_sample(seed, stream, (uint32_t)env, key, (uint32_t)idx, ch.distribution, ch.p0[comp], ch.p1[comp]));
}
// contact-material channel (include/lm_engine.h, LM_DR_MATERIALS): the dynamic coefficient of one surface.  on_startup entries are keyed by
// (seed, channel, env) only; with K buckets the channel's one uniform variate is quantised to the midpoints of K equal cells before it is
// mapped through the distribution (the inverse normal CDF for gaussian), so a channel has at most K distinct values
#define LM_DR_STREAM_MAT 10U      // streams 10, 11 (0..8: the channels above, 9: action sampling)
#define LM_DR_STREAM_RESET 12U    // streams 12..15: the reset-state channels (LM_DR_RESET_*)
LM_DEV float dr_material(const lm_dr_channel& ch, int buckets, uint32_t seed, uint32_t stream, int env, uint32_t dr_step, uint32_t reset_key, float base) {
  if (!ch.enabled) return base;
  const uint32_t key = ch.interval > 0 ? dr_step / (uint32_t)ch.interval : (ch.interval < 0 ? 0U : reset_key);
  if (ch.interval == 0 && key == 0) return base;
  float n;
  if (buckets > 0) {
    float u1, u2; lm_rng_pair(lm_rng_base(seed, stream, (uint32_t)env, key), 0, &u1, &u2);
    const float K = (float)buckets, uq = (fminf(floorf(u2 * K), K - 1.0f) + 0.5f) / K;
    const float p0 = ch.p0[1], p1 = ch.p1[1];
    n = ch.distribution == LM_DR_UNIFORM ? p0 + (p1 - p0) * uq
      : ch.distribution == LM_DR_LOGUNIFORM ? expf(logf(p0) + (logf(p1) - logf(p0)) * uq)
      : p0 + p1 * (1.41421356237309505f * erfinvf(2.0f * uq - 1.0f));
  } else {
    n = dr_sample(seed, stream, (uint32_t)env, key, 1U, ch.distribution, ch.p0[1], ch.p1[1]);      // component 1 = dynamic
  }
  return dr_apply(ch.operation, base, n);
}
LM_DEV float friction_combine(int mode, float a, float b) {
  return mode == LM_COMBINE_AVERAGE ? 0.5f * (a + b) : mode == LM_COMBINE_MIN ? fminf(a, b) : mode == LM_COMBINE_MULTIPLY ? a * b : fmaxf(a, b);
}
// mass channel (include/lm_engine.h, LM_DR_MASS_CHANNELS): operation(nominal, draw) floored at LM_DR_MASS_FLOOR x nominal.  Keys as for the
// material channels; `comp` is the component of the draw (the body's index in table order), p0 / p1 its parameters
#define LM_DR_STREAM_MASS 16U     // streams 16 (plate mass), 17 (plate density), 18 (body masses)
LM_DEV float dr_mass(const lm_dr_channel& ch, uint32_t seed, uint32_t stream, int env, uint32_t dr_step, uint32_t reset_key, uint32_t comp, float p0, float p1, float base) {
  if (!ch.enabled) return base;
  const uint32_t key = ch.interval > 0 ? dr_step / (uint32_t)ch.interval : (ch.interval < 0 ? 0U : reset_key);
  if (ch.interval == 0 && key == 0) return base;
  return fmaxf(dr_apply(ch.operation, base, dr_sample(seed, stream, (uint32_t)env, key, comp, ch.distribution, p0, p1)), LM_DR_MASS_FLOOR * base);
}
struct DrPhys { float tmax[3], vmax[3], cj[3]; V3 g, f; float mu;      // this lane's three joints; gravity (world); base-link force (world); contact mu
                // mass channels: wave-uniform switches (bodies / plate); masses of the shell, (link4 | link1), (link3 | link2) and the hub; the plate's
                // mass and the factor on its inertia about the COM.  Read only where the matching switch is on
                int mb_on, mp_on; float m_s; f2 m_41, m_32; float m_hub, m_plate, s_plate;
                // actuator channels: this env's velocity gain kd and kp / kd (the block's values while the gain channels are off); lat_on: the
                // latency channel is on (wave-uniform), lat: the sub-steps of this step that still follow the previous command
                float kd, gk; int lat_on, lat; };
// actuator channels (include/lm_engine.h, LM_DR_ACTUATOR_CHANNELS): the gains go through dr_mass (floored at LM_DR_MASS_FLOOR x nominal); the
// latency is operation(0, draw), floored to whole sub-steps and clamped to [0, nsub]
#define LM_DR_STREAM_ACTUATOR 19U     // streams 19 (kp), 20 (kd), 21 (command latency)
LM_DEV int dr_latency(const lm_dr_channel& ch, uint32_t seed, int env, uint32_t dr_step, uint32_t reset_key, int nsub) {
  const uint32_t key = ch.interval > 0 ? dr_step / (uint32_t)ch.interval : (ch.interval < 0 ? 0U : reset_key);
  if (ch.interval == 0 && key == 0) return 0;
  const float x = dr_apply(ch.operation, 0.f, dr_sample(seed, LM_DR_STREAM_ACTUATOR + LM_DR_ACTUATOR_LATENCY, (uint32_t)env, key, 0U, ch.distribution, ch.p0[0], ch.p1[0]));
  return (int)fminf(fmaxf(floorf(x), 0.f), (float)nsub);
}
