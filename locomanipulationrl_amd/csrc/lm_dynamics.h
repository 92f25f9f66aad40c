// lm_dynamics.h -- device code of the step, layer 2 of 4: table and state layout, limb kinematics and dynamics, the hub Cholesky solve, the
// contact PGS, the LDS stash and one physics sub-step.  The device globals of the diagnostic builds (lm_stamp_lds of LM_STAMPS,
// lm_dbg_pass2 of LM_COUNT_PASS2) are defined by lm_engine.hip before it includes this file; lm_engine_w2.hip drops both switches.
#pragma once
#include "lm_samplers.h"

// Diagnostic build only (-DLM_STAMPS, tools/stamp_profile.sh): LM_STAMP(k) adds the shader cycles since the previous stamp to bucket k of
// a per-workgroup LDS array (lm_stamp_lds, defined in lm_engine.hip) that k_step copies to lm_stamp_out.  No stamp exists in the product build.
#if defined(LM_STAMPS) && LM_STAMPS != 2      // 2: only the wavefront's lifetime (two clock reads around the whole body): what the product code takes inside the kernel
#define LM_STAMP(k) do { __builtin_amdgcn_sched_barrier(0); unsigned long long t_; \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); __builtin_amdgcn_sched_barrier(0); \
    if (threadIdx.x == 0) { lm_stamp_lds[k] += t_ - lm_stamp_lds[15]; lm_stamp_lds[15] = t_; } } while (0)
#else
#define LM_STAMP(k) do { } while (0)
#endif

#define HUB_FLOATS 10
#define ENVS_PER_WAVE 16
// Device-side table layout (built from the packed public table by permute_table() in lm_create).  A limb is the shell plus two
// structurally identical two-link chains, A = link4 -> link3 (joints dof2, p1) and B = link1 -> link2 (joints dof3, p2); the entries
// of the chains are interleaved (A, B) so that one 8-byte LDS read feeds one packed-fp32 operand (lm_math.h).
#define PUB_LIMB_STRIDE 123   // public: 5 joints x 13, 5 inertias x 10, tip (3), foot-sphere centre (3), foot body flag, pad
#define LIMB_STRIDE 124       // device: even, every pair 8-byte aligned
#define T_J0 0                // shell joint: R (9, row-major), p (3), axis sign
#define T_P1 14               // 13 pairs: first joints of the chains (dof2 | dof3)
#define T_P2 40               // 13 pairs: second joints (p1 | p2)
#define T_I0 66               // shell inertia (m, com 3, I 6)
#define T_Q1 76               // 10 pairs: link4 | link1
#define T_Q2 96               // 10 pairs: link3 | link2
#define T_TIP 116             // fingertip frame on link3
#define T_FOOT 119            // foot-sphere centre in its body's frame
#define T_FLAG 122            // 0: the foot rides on link3, 1: on link2
#define LM_ITAB_FLOATS (HUB_FLOATS + 4 * LIMB_STRIDE)

// state rows
#define R_FB0 0            // base: pos 0..2 quat 3..6 lin 7..9 ang 10..12
#define R_Q 13
#define R_QD 25
#define R_FB1 37           // plate: pos, quat, lin, ang
#define R_LACT 50
#define R_LQD 62
#define R_LTIP 74
#define R_GOAL 86
#define R_SE 90           // swing/extension position targets (custom-controller tasks)
#define R_LTGT 102        // last joint position targets
#define R_LRD 114         // last rot_dist

#define SQRT2F 1.41421356237f

LM_DEV Q4 quat_from_euler(float roll, float pitch, float yaw) {
  float sy, cy, sr, cr, sp, cp;
  sincosf(yaw * 0.5f, &sy, &cy); sincosf(roll * 0.5f, &sr, &cr); sincosf(pitch * 0.5f, &sp, &cp);
  Q4 q; q.w = cy * cr * cp + sy * sr * sp; q.x = cy * sr * cp - sy * cr * sp; q.y = cy * cr * sp + sy * sr * cp; q.z = sy * cr * cp - cy * sr * sp;
  return q;
}
LM_DEV M3 load_m3_rowmajor(const float* t) {
  M3 R; R.c0 = v3(t[0], t[3], t[6]); R.c1 = v3(t[1], t[4], t[7]); R.c2 = v3(t[2], t[5], t[8]); return R;
}
LM_DEV SI load_si(const float* t) { SI I; I.m = t[0]; I.h = v3(t[1], t[2], t[3]); I.xx = t[4]; I.yy = t[5]; I.zz = t[6]; I.xy = t[7]; I.xz = t[8]; I.yz = t[9]; return I; }
// hub body: the device table holds its spatial inertia about the hub origin (permute_table)
LM_DEV SI hub_inertia(const float* t) { return load_si(t); }
LM_DEV void si_to_66(const SI& I, float A[6][6]) {
  A[0][0] = I.xx; A[0][1] = I.xy; A[0][2] = I.xz; A[1][1] = I.yy; A[1][2] = I.yz; A[2][2] = I.zz;
  A[1][0] = I.xy; A[2][0] = I.xz; A[2][1] = I.yz;
  // M_wv = [h]x, M_vw = -[h]x
  A[0][3] = 0.f;     A[0][4] = -I.h.z; A[0][5] = I.h.y;
  A[1][3] = I.h.z;   A[1][4] = 0.f;    A[1][5] = -I.h.x;
  A[2][3] = -I.h.y;  A[2][4] = I.h.x;  A[2][5] = 0.f;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) { A[3 + i][j] = A[j][3 + i]; A[3 + i][3 + j] = (i == j) ? I.m : 0.f; }
}
LM_DEV void sv_to_arr(SV a, float* o) { o[0] = a.w.x; o[1] = a.w.y; o[2] = a.w.z; o[3] = a.v.x; o[4] = a.v.y; o[5] = a.v.z; }
LM_DEV SV arr_to_sv(const float* o) { return sv(v3(o[0], o[1], o[2]), v3(o[3], o[4], o[5])); }

// one joint of the limb tree: parent pose (Rp, op) + table entry (R 9 row-major, p 3, sign) + rotation (c, s); T = float for the shell
// joint, f2 for a pair of chain joints (table entries interleaved)
template <class T> LM_DEV M3T<T> load_m3_rowmajor_t(const T* t) {
  M3T<T> R; R.c0 = v3t<T>(t[0], t[3], t[6]); R.c1 = v3t<T>(t[1], t[4], t[7]); R.c2 = v3t<T>(t[2], t[5], t[8]); return R;
}
template <class T> LM_DEV void joint_frame(const M3T<T>& Rp, V3T<T> op, const T* tj, T c, T s, M3T<T>& R, V3T<T>& o, V3T<T>& z) {
  M3T<T> A = mul(Rp, load_m3_rowmajor_t<T>(tj));
  T sg = tj[12]; T ss = sg * s;
  R.c0 = fma3(c, A.c0, ss * A.c1);
  R.c1 = fma3(c, A.c1, (-ss) * A.c0);
  R.c2 = A.c2;
  o = op + mul(Rp, v3t<T>(tj[9], tj[10], tj[11]));
  z = sg * A.c2;
}
// the shell joint hangs on the hub frame itself (identity parent): no parent products
LM_DEV void joint_frame_root(const float* tj, float c, float s, M3& R, V3& o, V3& z) {
  M3 A = load_m3_rowmajor_t<float>(tj);
  float sg = tj[12]; float ss = sg * s;
  R.c0 = fma3(c, A.c0, ss * A.c1);
  R.c1 = fma3(c, A.c1, (-ss) * A.c0);
  R.c2 = A.c2;
  o = v3(tj[9], tj[10], tj[11]);
  z = sg * A.c2;
}
// sin/cos of a pair of angles (same polynomial as lm_sincos, both halves in packed instructions where the ISA has them)
LM_DEV void lm_sincos2(f2 x, f2* s, f2* c) {
  const f2 kf = mk2(rintf(x.x * 0.636619772367581343f), rintf(x.y * 0.636619772367581343f));
  const int k0 = (int)kf.x, k1 = (int)kf.y;
  f2 r = fma_(-kf, sp2(1.57079625129699707031f), x);
  r = fma_(-kf, sp2(7.54978941586159635335e-8f), r);
  r = fma_(-kf, sp2(5.39030285815811905290e-15f), r);
  const f2 z = r * r;
  const f2 sp = fma_(fma_(fma_(sp2(-1.9515295891e-4f), z, sp2(8.3321608736e-3f)), z, sp2(-1.6666654611e-1f)), z * r, r);
  const f2 cp = fma_(fma_(fma_(sp2(2.443315711809948e-5f), z, sp2(-1.388731625493765e-3f)), z, sp2(4.166664568298827e-2f)), z * z, fma_(sp2(-0.5f), z, sp2(1.0f)));
  const float ss0 = (k0 & 1) ? cp.x : sp.x, cc0 = (k0 & 1) ? sp.x : cp.x, ss1 = (k1 & 1) ? cp.y : sp.y, cc1 = (k1 & 1) ? sp.y : cp.y;
  *s = mk2((k0 & 2) ? -ss0 : ss0, (k1 & 2) ? -ss1 : ss1);
  *c = mk2(((k0 + 1) & 2) ? -cc0 : cc0, ((k1 + 1) & 2) ? -cc1 : cc1);
}

// kinematics + dynamics terms of one limb, all in hub ("base") coordinates about the hub origin.  Pairs hold (chain A | chain B) =
// (link4 | link1) at the first level and (link3 | link2) at the second.
struct LimbKin {
  M3 Rs; V3 os; SV s1;                     // shell
  M3P R41, R32; V3P o41, o32;              // frames: (link4 | link1), (link3 | link2); tip on link3, knees = origins of link3 and link2
  SVP s23, sp12;                           // joint axes (dof2 | dof3), (p1 | p2)
  float g1, pd, pdd;                       // closure: dp/dD, passive rate, passive vp-acceleration
};

LM_DEV void limb_kinematics(const float* tl, const float q[3], const float qd[3], LimbKin& K) {
  float s1_, c1_; f2 s23_, c23_;
  lm_sincos(q[0], &s1_, &c1_); lm_sincos2(mk2(q[1], q[2]), &s23_, &c23_);
  const float s2_ = s23_.x, c2_ = c23_.x, s3_ = s23_.y, c3_ = c23_.y;
  float cD = c2_ * c3_ + s2_ * s3_, sD = s2_ * c3_ - c2_ * s3_;      // D = q2 - q3
  float inv = 1.0f / (3.0f - cD);
  float cp = (3.0f * cD - 1.0f) * inv, sp = 2.0f * SQRT2F * sD * inv;
  K.g1 = 2.0f * SQRT2F * inv;
  float g2 = -2.0f * SQRT2F * sD * inv * inv;
  float dd = qd[1] - qd[2];
  K.pd = K.g1 * dd; K.pdd = g2 * dd * dd;
  const f2* tp = reinterpret_cast<const f2*>(tl);
  V3 z1; V3P z23, zp12;
  joint_frame_root(tl + T_J0, c1_, s1_, K.Rs, K.os, z1);
  joint_frame<f2>(bc(K.Rs), bc(K.os), tp + T_P1 / 2, c23_, s23_, K.R41, K.o41, z23);          // dof2 | dof3
  joint_frame<f2>(K.R41, K.o41, tp + T_P2 / 2, sp2(cp), mk2(sp, -sp), K.R32, K.o32, zp12);    // p1 = +g(D) | p2 = -g(D)
  K.s1 = axis_sv(z1, K.os); K.s23 = axis_sv(z23, K.o41); K.sp12 = axis_sv(zp12, K.o32);
}
// the fingertip frame (on link3) and the two knee origins of a limb, hub coordinates
LM_DEV void limb_points(const float* tl, const LimbKin& K, V3& tip, V3& knee2, V3& knee3) {
  knee3 = lo(K.o32); knee2 = hi(K.o32);
  tip = knee3 + mul(lo(K.R32), v3(tl[T_TIP], tl[T_TIP + 1], tl[T_TIP + 2]));
}

struct LimbDyn {
  SV Fq0, Fq1, Fq2;       // coupling columns (6x3): hub wrench per unit limb acceleration
  float H[6];             // limb joint-space inertia, packed [00,01,02,11,12,22]
  float hq[3];            // limb bias
  SV fcs;                 // limb bias wrench on the hub
  SI Isc;                 // limb composite inertia
  SV j31, j32;            // motion of the foot's body (link3, or link2 on a right-hand module) per unit rate of (q2, q3); per unit q1 it is s1
  V3 x;                   // centre of the foot sphere (hub coords)
};
LM_DEV V3 sel(bool c, V3 a, V3 b) { return v3(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }
LM_DEV SV sel(bool c, SV a, SV b) { return sv(sel(c, a.w, b.w), sel(c, a.v, b.v)); }

// MASS = 1 (the randomised kernels with the body-mass channel on): the masses of the five bodies come from the caller instead of the table;
// COM and inertia about the COM stay the table's
// PART (k_step_h2, lm_engine_h2.hip): 0 = both chains below; 1 = the inertia chain only (wavefront 0: fcs and hq are left unset and come from the
// helper wavefront through LDS); 2 = the bias chain only (the helper: only fcs and hq are set).  After the placed inertias the chains share no
// value, and each is compiled from the lines every other kernel compiles
template <int MASS = 0, int PART = 0>
LM_DEV void limb_dynamics(const float* tl, const LimbKin& K, const float qd[3], SV v0, SV avp0, LimbDyn& D, float m_s = 0.f, f2 m_41 = f2{0.f, 0.f}, f2 m_32 = f2{0.f, 0.f}) {
  const f2* tp = reinterpret_cast<const f2*>(tl);
  const SI Is = MASS ? place_inertia_m<float>(tl + T_I0, m_s, K.Rs, K.os) : place_inertia<float>(tl + T_I0, K.Rs, K.os);
  const SIP I41 = MASS ? place_inertia_m<f2>(tp + T_Q1 / 2, m_41, K.R41, K.o41) : place_inertia<f2>(tp + T_Q1 / 2, K.R41, K.o41),
            I32 = MASS ? place_inertia_m<f2>(tp + T_Q2 / 2, m_32, K.R32, K.o32) : place_inertia<f2>(tp + T_Q2 / 2, K.R32, K.o32);
  if (PART != 1) {
  // velocities / velocity-product accelerations down the two chains
  const SV j1 = qd[0] * K.s1; const SVP j23 = mk2(qd[1], qd[2]) * K.s23, jp = mk2(K.pd, -K.pd) * K.sp12;
  const SV vs = v0 + j1; const SVP v41 = bc(vs) + j23, v32 = v41 + jp;
  const SV as = avp0 + mcross(v0, j1);
  const SVP a41 = bc(as) + mcross(bc(vs), j23);
  const SVP a32 = fma6(mk2(K.pdd, -K.pdd), K.sp12, a41 + mcross(v41, jp));
  // bias wrenches
  const SV ps = Is * as + fcross(vs, Is * vs);
  const SVP p41 = I41 * a41 + fcross(v41, I41 * v41), p32 = I32 * a32 + fcross(v32, I32 * v32);
  const SVP fc = p41 + p32;                                             // (fc4 | fc1)
  D.fcs = ps + lo(fc) + hi(fc);
  const float h1 = sdot(K.s1, D.fcs); const f2 h23 = sdot(K.s23, fc), hp = sdot(K.sp12, p32);      // (h2 | h3), (hp1 | hp2)
  const float g1 = K.g1, dh = hp.x - hp.y;
  D.hq[0] = h1; D.hq[1] = h23.x + g1 * dh; D.hq[2] = h23.y - g1 * dh;
  }
  if (PART == 2) return;
  const float g1 = K.g1;
  // composite inertias and the columns of the coupling / joint-space inertia
  const SIP Ic = I41 + I32;                                             // (I4c | I1c)
  D.Isc = Is + lo(Ic) + hi(Ic);
  const SV F1 = D.Isc * K.s1; const SVP F23 = Ic * K.s23, Fp = I32 * K.sp12;      // (F2 | F3), (Fp1 | Fp2)
  const SV dF = lo(Fp) - hi(Fp);
  D.Fq0 = F1; D.Fq1 = fma6(g1, dF, lo(F23)); D.Fq2 = fma6(-g1, dF, hi(F23));
  const SVP s1p = bc(K.s1);
  const float H11 = sdot(K.s1, F1);
  const f2 H1d = sdot(s1p, F23), H1p = sdot(s1p, Fp);                   // (H12 | H13), (H1p1 | H1p2)
  const f2 Hdd = sdot(K.s23, F23), Hdp = sdot(K.s23, Fp), Hpp = sdot(K.sp12, Fp);      // (H22 | H33), (H2p1 | H3p2), (Hp1p1 | Hp2p2)
  const float gg = g1 * g1 * (Hpp.x + Hpp.y), d1p = H1p.x - H1p.y;
  D.H[0] = H11; D.H[1] = H1d.x + g1 * d1p; D.H[2] = H1d.y - g1 * d1p;
  D.H[3] = Hdd.x + 2.0f * g1 * Hdp.x + gg; D.H[4] = -g1 * (Hdp.x + Hdp.y) - gg; D.H[5] = Hdd.y + 2.0f * g1 * Hdp.y + gg;
  // foot collider = the hemispherical end of the long distal link (robot_model.py FOOT_*): link3 (chain dof2 -> p1 = +g(D)) on a left-hand
  // module, link2 (chain dof3 -> p2 = -g(D)) on a right-hand one
  const bool on2 = tl[T_FLAG] != 0.f;
  const V3 off = v3(tl[T_FOOT], tl[T_FOOT + 1], tl[T_FOOT + 2]);
  const SV s2 = lo(K.s23), s3 = hi(K.s23), sp1 = lo(K.sp12), sp2_ = hi(K.sp12);
  D.j31 = sel(on2, (-g1) * sp2_, fma6(g1, sp1, s2));
  D.j32 = sel(on2, fma6(g1, sp2_, s3), (-g1) * sp1);
  D.x = sel(on2, hi(K.o32), lo(K.o32)) + mul(M3{sel(on2, hi(K.R32.c0), lo(K.R32.c0)), sel(on2, hi(K.R32.c1), lo(K.R32.c1)), sel(on2, hi(K.R32.c2), lo(K.R32.c2))}, off);
}

// Projected Gauss-Seidel over the 4 tip contacts of one env (rows n, t1, t2 per contact, limb order).
// The Delassus operator is  W_ij = delta_ij D_i + T_i^T Phi T_j  (arrowhead structure of the hub + limbs system).
// Each lane keeps the current contact-space velocity c (3) of ITS contact, its own full 3x3 block, and the 3x3
// cross blocks X_K = T_i^T B_K towards the other three contacts; lanes take turns, the lane whose turn it is
// relaxes its normal row and then its two friction rows together (one packed update: both see the state the normal row left,
// their mutual coupling enters at the contact's next turn; the pair is projected onto the friction cone), then its three impulse
// increments are quad-broadcast and every lane updates c.  Identical arithmetic (up to rounding) to the oracle's sweep over the dense 12x12 system.
// Row layout: row 0 (normal) in plain registers, rows 1 | 2 (friction) as one packed pair.
struct PgsData { f2 W0t, nrWt; float X0[4][3]; f2 X12[4][3]; };   // own block: (W01 | W02), (-1/(mu W11) | -1/(mu W22)); columns 1, 2 of the X blocks carry mu, row 0 (X0) is scaled by -1/W00 (the normal residual is carried as the unclamped impulse step);
                                                                                   // block towards contact K (K == own limb: the own block) by columns s: X0[K][s] = X[0][s], X12[K][s] = (X[1][s] | X[2][s])

// ---- "four 6-vectors at once" layout of the pass linear algebra.  Component i of the vectors (v0, v1, v2, v3) is an R4: p = (v0[i] | v1[i]),
// q = (v2[i] | v3[i]), so that an operation applied to all four is two packed-fp32 instructions and any single entry is a free half-register
// read.  The pass uses it for (-bA, T0, T1, T2) - the hub bias and the three contact rows of this lane - and for what the hub solve makes of
// them, (a0, B0, B1, B2).
struct R4 { f2 p, q; };
// component-pair layout of ONE 6-vector (w.x,w.y | w.z,v.x | v.y,v.z): what a float4 stash reload delivers in aligned register pairs
struct S6 { f2 a, b, c; };
LM_DEV S6 operator*(float s, S6 x) { const f2 t = sp2(s); S6 r; r.a = t * x.a; r.b = t * x.b; r.c = t * x.c; return r; }
LM_DEV S6 fma6(float s, S6 x, S6 y) { const f2 t = sp2(s); S6 r; r.a = fma_(t, x.a, y.a); r.b = fma_(t, x.b, y.b); r.c = fma_(t, x.c, y.c); return r; }
template <int I> LM_DEV float comp(const S6& x) { return I == 0 ? x.a.x : I == 1 ? x.a.y : I == 2 ? x.b.x : I == 3 ? x.b.y : I == 4 ? x.c.x : x.c.y; }
template <int J> LM_DEV f2 pairc(const S6& x) { return J == 0 ? x.a : J == 1 ? x.b : x.c; }

// Cholesky factor of a symmetric positive definite 6x6 matrix given by its upper triangle: L (strictly lower) and 1 / diagonal
struct Chol6 { float L[6][6]; float d[6]; };
LM_DEV void chol6(const float A[6][6], Chol6& C) {
#pragma unroll
  for (int j = 0; j < 6; j++) {
    float s = A[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) s = fmaf(-C.L[j][k], C.L[j][k], s);
    const float inv = __builtin_amdgcn_rsqf(s);      // v_rsq_f32 (1 ulp); the pivots are O(1e-3 .. 1): no denormal scaling needed
    C.d[j] = inv;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      float t = A[j][i];
#pragma unroll
      for (int k = 0; k < j; k++) t = fmaf(-C.L[i][k], C.L[j][k], t);
      C.L[i][j] = t * inv;
    }
  }
}
// A x = b for four right-hand sides at once, in place (forward then backward substitution: 84 packed instructions)
LM_DEV void chol6_solve4(const Chol6& C, R4 x[6]) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    f2 p = x[i].p, q = x[i].q;
#pragma unroll
    for (int k = 0; k < i; k++) { const f2 l = sp2(-C.L[i][k]); p = fma_(l, x[k].p, p); q = fma_(l, x[k].q, q); }
    const f2 d = sp2(C.d[i]); x[i].p = p * d; x[i].q = q * d;
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    f2 p = x[i].p, q = x[i].q;
#pragma unroll
    for (int k = i + 1; k < 6; k++) { const f2 l = sp2(-C.L[k][i]); p = fma_(l, x[k].p, p); q = fma_(l, x[k].q, q); }
    const f2 d = sp2(C.d[i]); x[i].p = p * d; x[i].q = q * d;
  }
}

// 3x3 block of this lane's contact rows T_i against the B vectors of contact K:  X[r][s] = T_i,r . B_K,s  (K == own limb: the own block)
// (in two steps: the raw block, and the select of the own block over it.  k_step_h3's helper wavefronts run the first step for wavefront 0,
// helper_xblocks below, and wavefront 0 the second on what they hand back)
struct XRaw { float a00; f2 a0t, c0, c1, c2; };      // row 0: column 0, columns (1 | 2); rows (1 | 2): columns 0, 1, 2
template <int K>
LM_DEV void pgs_cross_raw(const R4 T[6], const R4 X[6], XRaw& R) {
  float a00 = 0.f; f2 a0t = sp2(0.f), c0 = sp2(0.f), c1 = sp2(0.f), c2 = sp2(0.f);
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const float k0 = quad_bcast<K>(X[i].p.y); const f2 k12 = mk2(quad_bcast<K>(X[i].q.x), quad_bcast<K>(X[i].q.y));
    const float t0 = T[i].p.y; const f2 t12 = T[i].q;
    a00 = fmaf(t0, k0, a00); a0t = fma_(sp2(t0), k12, a0t);                                   // row 0: column 0, columns (1 | 2)
    c0 = fma_(t12, sp2(k0), c0); c1 = fma_(t12, sp2(k12.x), c1); c2 = fma_(t12, sp2(k12.y), c2);      // rows (1 | 2): columns 0, 1, 2
  }
  R.a00 = a00; R.a0t = a0t; R.c0 = c0; R.c1 = c1; R.c2 = c2;
}
template <int K>
LM_DEV void pgs_cross_select(int limb, const XRaw& R, const float Wf[6], float X0[3], f2 X12[3]) {
  const bool own = (limb == K);
  X0[0] = own ? Wf[0] : R.a00; X0[1] = own ? Wf[1] : R.a0t.x; X0[2] = own ? Wf[2] : R.a0t.y;
  X12[0] = mk2(own ? Wf[1] : R.c0.x, own ? Wf[2] : R.c0.y);
  X12[1] = mk2(own ? Wf[3] : R.c1.x, own ? Wf[4] : R.c1.y);
  X12[2] = mk2(own ? Wf[4] : R.c2.x, own ? Wf[5] : R.c2.y);
}
template <int K>
LM_DEV void pgs_cross_blocks(int limb, const R4 T[6], const R4 X[6], const float Wf[6], float X0[3], f2 X12[3]) {
  XRaw R; pgs_cross_raw<K>(T, X, R); pgs_cross_select<K>(limb, R, Wf, X0, X12);
}

// One Gauss-Seidel turn: contact K relaxes its normal row, then its two friction rows as a pair (both from the state the normal row
// left), then its three impulse increments are quad-broadcast and EVERY lane, the owner included, applies c += X[K] * d.  Lanes whose
// turn it is not run the same instructions on their own (discarded) candidates; the impulses move by  m * d  with m = 1 on the owner
// lane and 0 elsewhere (one FMA instead of an add and a select).  The friction impulses are carried divided by mu, so that their bound
// is the normal impulse itself and mu sits in the constants (nrWt, columns 1 and 2 of the X blocks).
// Measured alternatives (tools/ab_build.py, profiles/r03_pgs_turn_ab.json): the relaxation as a real branch under the owner lanes'
// execution mask (18 vector + 3 scalar instructions per turn) is 14 % SLOWER per sweep than selects (20 vector instructions).
template <int K>
LM_DEV void pgs_turn(float m, const PgsData& G, float& lam0, f2& lam12, float& c0, f2& c12) {
  const float d0 = __builtin_amdgcn_fmed3f(c0, -lam0, __builtin_inff());               // max(-lam0, -v_n / W00): c0 is carried as -v_n / W00 (one v_max, no canonicalising copy of -lam0)
  lam0 = fmaf(m, d0, lam0);                                                            // owner: the relaxed normal impulse, which bounds its friction rows
  const f2 u12 = fma_(fma_(G.W0t, sp2(d0), c12), G.nrWt, lam12);
  // projection of the friction pair onto the cone |lam_t| <= mu lam_n (here: |u| <= lam0, the pair being carried divided by mu): scale by
  // min(1, lam0 / |u|).  |u| = 0 gives lam0 * inf = inf (or NaN when lam0 = 0 too), and v_min returns 1 for both
  const float sc = fminf(1.0f, lam0 * __builtin_amdgcn_rsqf(fmaf(u12.x, u12.x, u12.y * u12.y)));
  const f2 d12 = fma_(u12, sp2(sc), -lam12);
  lam12 = fma_(sp2(m), d12, lam12);
  const float b0 = quad_bcast<K>(d0), b1 = quad_bcast<K>(d12.x), b2 = quad_bcast<K>(d12.y);
  // the normal increment's terms first: they are ready before the friction pair's broadcasts and fill those broadcasts' wait states
  c0 = fmaf(G.X0[K][2], b2, fmaf(G.X0[K][1], b1, fmaf(G.X0[K][0], b0, c0)));
  c12 = fma_(G.X12[K][2], sp2(b2), fma_(G.X12[K][1], sp2(b1), fma_(G.X12[K][0], sp2(b0), c12)));
}

// T[i].p.y, T[i].q = this lane's three contact rows (hub / plate wrench per unit impulse); X[i].p.y, X[i].q = B = Phi T
struct PgsState { PgsData G; float lam0; f2 lam12; float c0; f2 c12; float m0, m1, m2, m3; };
#ifndef LM_H3_XBLOCKS
#define LM_H3_XBLOCKS 0
#endif
struct Stash;
#if defined(LM_HELPER_WAVE) && LM_HELPER_WAVE >= 2
LM_DEV void xblocks_fetch(const Stash* Hd, XRaw& R0, XRaw& R1, XRaw& R2, XRaw& R3);      // (with the helpers, below)
#endif
// a value computed here and now: the optimiser neither sinks its computation behind a later barrier nor sees through it
LM_DEV void pin_here(float& x) { asm volatile("" : "+v"(x)); }
LM_DEV void pin_here(f2& x) { asm volatile("" : "+v"(x)); }
// XB (the first pass of wavefront 0 of k_step_h3, LM_H3_XBLOCKS): the four raw cross blocks are the helper wavefronts', fetched behind barrier B3
template <int XB = 0>
LM_DEV void pgs_setup(PgsState& S, int limb, float mu, float bn, const float vf[3], const float Wl[6], const R4 T[6], const R4 X[6], const Stash* Hd = nullptr) {
  PgsData& G = S.G; float Wf[6];
  // full own block = limb-local part + hub/plate part T_r^T Phi T_s
  {
    f2 a0 = sp2(0.f), a1 = sp2(0.f), a2 = sp2(0.f); float b0 = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      b0 = fmaf(T[i].p.y, X[i].p.y, b0);
      a0 = fma_(sp2(T[i].p.y), X[i].q, a0); a1 = fma_(sp2(T[i].q.x), X[i].q, a1); a2 = fma_(sp2(T[i].q.y), X[i].q, a2);
    }
    Wf[0] = Wl[0] + b0; Wf[1] = Wl[1] + a0.x; Wf[2] = Wl[2] + a0.y;
    Wf[3] = Wl[3] + a1.x; Wf[4] = Wl[4] + a1.y; Wf[5] = Wl[5] + a2.y;
  }
  // friction impulses are carried as lam_t / mu (bound = the normal impulse); mu = 0 pins them at zero
  const float imu = mu > 0.f ? 1.0f / mu : 0.f;
  float nrW0 = -1.0f / Wf[0]; G.W0t = mk2(Wf[1], Wf[2]); G.nrWt = mk2(-imu / Wf[3], -imu / Wf[5]);
#if defined(LM_HELPER_WAVE) && LM_HELPER_WAVE >= 2
  if (XB) {
    // all that is this wavefront's own stands in front of B3 (left to the optimiser, the own block is sunk behind the barrier, to its first use);
    // behind it: the reads, the selects and the scaling
    S.c0 = (vf[0] + bn) * nrW0; S.c12 = mk2(vf[1], vf[2]);
    pin_here(Wf[0]); pin_here(Wf[1]); pin_here(Wf[2]); pin_here(Wf[3]); pin_here(Wf[4]); pin_here(Wf[5]);
    pin_here(nrW0); pin_here(G.nrWt); pin_here(S.c0); pin_here(S.c12);
    XRaw R0, R1, R2, R3; xblocks_fetch(Hd, R0, R1, R2, R3);
    pgs_cross_select<0>(limb, R0, Wf, G.X0[0], G.X12[0]); pgs_cross_select<1>(limb, R1, Wf, G.X0[1], G.X12[1]);
    pgs_cross_select<2>(limb, R2, Wf, G.X0[2], G.X12[2]); pgs_cross_select<3>(limb, R3, Wf, G.X0[3], G.X12[3]);
  } else
#endif
  {
  pgs_cross_blocks<0>(limb, T, X, Wf, G.X0[0], G.X12[0]); pgs_cross_blocks<1>(limb, T, X, Wf, G.X0[1], G.X12[1]);
  pgs_cross_blocks<2>(limb, T, X, Wf, G.X0[2], G.X12[2]); pgs_cross_blocks<3>(limb, T, X, Wf, G.X0[3], G.X12[3]);
  }
#pragma unroll
  for (int k = 0; k < 4; k++) { G.X0[k][0] *= nrW0; G.X0[k][1] *= mu * nrW0; G.X0[k][2] *= mu * nrW0; G.X12[k][1] = sp2(mu) * G.X12[k][1]; G.X12[k][2] = sp2(mu) * G.X12[k][2]; }
  S.lam0 = 0.f; S.lam12 = sp2(0.f);
  if (!XB) { S.c0 = (vf[0] + bn) * nrW0; S.c12 = mk2(vf[1], vf[2]); }
  S.m0 = limb == 0 ? 1.f : 0.f; S.m1 = limb == 1 ? 1.f : 0.f; S.m2 = limb == 2 ? 1.f : 0.f; S.m3 = limb == 3 ? 1.f : 0.f;
}
// sweeps it0 (even) ... it1 - 1.  Sweeps alternate direction (contacts 0,1,2,3 then 3,2,1,0): no limb is systematically relaxed first,
// which removes the ordering bias an unconverged Gauss-Seidel solve would otherwise leave between the four limbs
LM_DEV void pgs_sweeps(PgsState& S, int it0, int it1) {
  for (int it = it0; it < it1; it += 2) {
    pgs_turn<0>(S.m0, S.G, S.lam0, S.lam12, S.c0, S.c12);
    pgs_turn<1>(S.m1, S.G, S.lam0, S.lam12, S.c0, S.c12);
    pgs_turn<2>(S.m2, S.G, S.lam0, S.lam12, S.c0, S.c12);
    pgs_turn<3>(S.m3, S.G, S.lam0, S.lam12, S.c0, S.c12);
    if (it + 1 < it1) {
      pgs_turn<3>(S.m3, S.G, S.lam0, S.lam12, S.c0, S.c12);
      pgs_turn<2>(S.m2, S.G, S.lam0, S.lam12, S.c0, S.c12);
      pgs_turn<1>(S.m1, S.G, S.lam0, S.lam12, S.c0, S.c12);
      pgs_turn<0>(S.m0, S.G, S.lam0, S.lam12, S.c0, S.c12);
    }
  }
}
// impulses found so far and the hub / plate velocity change  w = Phi sum_j T_j lam_j = sum_j B_j lam_j
LM_DEV void pgs_finish(const PgsState& S, float mu, const R4 X[6], float lam[3], float w[6]) {
  const f2 l12 = sp2(mu) * S.lam12;
  lam[0] = S.lam0; lam[1] = l12.x; lam[2] = l12.y;
#pragma unroll
  for (int i = 0; i < 6; i++) { const f2 t = l12 * X[i].q; w[i] = quad_sum(fmaf(S.lam0, X[i].p.y, t.x + t.y)); }
}

// free rigid body carried as (position, quaternion, body-coordinate spatial velocity about its origin)
struct FreeBody { V3 p; Q4 q; SV u; };

LM_DEV void integrate_free(FreeBody& F, const M3& R, float dt) {
  V3 ww = mul(R, F.u.w);
  float wn = sqrtf(dot(ww, ww)), th = wn * dt;
  Q4 dq;
  if (th < 1e-8f) { dq.w = 1.f; dq.x = 0.5f * dt * ww.x; dq.y = 0.5f * dt * ww.y; dq.z = 0.5f * dt * ww.z; }
  else { float sh, ch; lm_sincos(0.5f * th, &sh, &ch); float s = sh / wn; dq.w = ch; dq.x = s * ww.x; dq.y = s * ww.y; dq.z = s * ww.z; }
  Q4 qn = qmul(dq, F.q);
  float rn = rsqrtf(qn.w * qn.w + qn.x * qn.x + qn.y * qn.y + qn.z * qn.z);
  F.q.w = qn.w * rn; F.q.x = qn.x * rn; F.q.y = qn.y * rn; F.q.z = qn.z * rn;
  M3 Rn = quat_to_mat(F.q.w, F.q.x, F.q.y, F.q.z);
  F.p = fma3(dt, mul(Rn, F.u.v), F.p);
}

// Per-lane stash in LDS for the pass-invariant terms of a sub-step (the SECOND drive pass needs them again after the contact
// iterations of the first; keeping them in registers across the PGS loop spills.  The first pass runs on the registers
// they were computed in, see PassTerms; k_step_w2 and the persistent rollouts read them back in both passes).
// Layout [slot][lane] as float4 -> conflict-free 16-byte accesses.
#ifdef LM_WAVES2
// k_step compiled for TWO wavefronts per SIMD.  That needs <= 256 registers per lane (amdgpu_waves_per_eu(2, 2): the
// compiler spills the rest to scratch) and <= 20 KB of LDS per wavefront (8 blocks per CU): the stash shrinks to 18 slots (the limb's last two
// inertia entries ride in the free half of slot 4) and the output staging (sObs, sSt: dead until the task layer, when the stash is dead) lives in
// the stash's memory.  Same arithmetic in the same order, so the same bits (tests/test_gpu_full_size.py).  The product compiles it as a SECOND
// translation unit (lm_engine_w2.hip: k_step_w2, the locomotion specialisation only) that lm_step dispatches beyond 32 768 envs - more than two
// generations of one-wavefront workgroups - for un-randomised velocity-drive locomotion engines: slower below (16 384 envs: 45 against 39 us),
// even at 24 576 / 32 768, + 5-8 % from 36 864, + 9 % at 65 536, + 14 % at 131 072, + 18 % at 262 144.
// (-DLM_WAVES2 on the whole library, tools/ab_build.py, is the A/B build of round 4: every step kernel then has this layout.)
#define STASH_SLOTS 18
#define LM_STEP_ATTR __attribute__((amdgpu_waves_per_eu(2, 2)))
#elif defined(LM_HELPER_WAVE)
// k_step_h2 (lm_engine_h2.hip): a second wavefront of the workgroup computes the limb bias terms (see helper_wave below).  The two wavefronts
// exchange 16 + 9 floats per lane and sub-step through seven more slots of the same [slot][lane] array.  k_step_h3 (lm_engine_h3.hip,
// LM_HELPER_WAVE 2) has a third wavefront for the contact terms (helper_wave_terms): it reads the same four slots, with the base height in
// the last word, and writes stash slots 7-15 themselves.  The task-layer state that wavefront 1 fetches during the last sub-step
// (helper_task_state, lm_step.h) has five slots of its own, TASK_SLOT: a second pass of that sub-step still reads slots 0-18 and HAND_OUT
#if LM_HELPER_WAVE >= 2
#define TASK_SLOT 29          // 5 slots, wavefront 1 -> wavefront 0: succ, consec, greset, reset | progress, episode, lact | lact, lqd | ltip, goal | goal
#if LM_H3_XBLOCKS
// The cross blocks of the contact operator on the helpers (helper_xblocks).  Hand-in, 10 slots, wavefront 0 -> helpers in front of the second
// barrier: K0 K1 K2 | the factor's d | its strictly lower L.  Its first five slots are TASK_SLOT's: the helpers have read them when they pass B3,
// wavefront 1 writes the task-layer state behind its last B3, and no second pass reads either.  Hand-back, 5 slots per helper, read by
// wavefront 0 behind B3: two raw blocks of 9 floats, wavefront 2's (contacts 0, 1) first
#define STASH_SLOTS 49
#define XB_IN_A TASK_SLOT     // 5 slots: K0 | K0, K1 | K1 | K2 | K2, d0, d1
#define XB_IN_B 34            // 5 slots: d2..d5 | L10 L20 L21 L30 | L31 L32 L40 L41 | L42 L43 L50 L51 | L52 L53 L54
#define XB_OUT 39             // 2 x 5 slots: a00, a0t, c0.x | c0.y, c1, c2.x | c2.y, a00', a0t' | c0', c1' | c2'
#else
#define STASH_SLOTS 34
#endif
#else
#define STASH_SLOTS 29
#endif
#define HAND_IN 22            // 4 slots, wavefront 0 -> helpers: q, qd | qd, u.w | u.w, u.v | row 2 of the base's rotation (k_step_h3: and the base height)
#define HAND_OUT 26           // 3 slots, helper -> wavefront 0: fcs | fcs, hq | hq
#define LM_STEP_ATTR
#else
#define STASH_SLOTS 22
#define LM_STEP_ATTR
#endif
struct Stash {
  float4* base; int lane;
  LM_DEV void put(int slot, float a, float b, float c, float d) const { base[slot * 64 + lane] = make_float4(a, b, c, d); }
  LM_DEV float4 get(int slot) const { return base[slot * 64 + lane]; }
};
#ifdef LM_HELPER_WAVE
// Workgroup barrier of k_step_h2 for data exchanged through LDS: waits for this wavefront's LDS operations only (not for loads and stores in
// flight), and keeps the scheduler from moving arithmetic across it - wavefront 0 is to do all the work that does not need the helper's
// result BEFORE it waits for that result.
LM_DEV void hw_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
#endif
LM_DEV void stash_sv3(const Stash& S, int slot, SV a, SV b, SV c, float e0 = 0.f, float e1 = 0.f) {      // 18 floats -> 5 slots (the last one half used: e0, e1 ride there)
  S.put(slot + 0, a.w.x, a.w.y, a.w.z, a.v.x); S.put(slot + 1, a.v.y, a.v.z, b.w.x, b.w.y);
  S.put(slot + 2, b.w.z, b.v.x, b.v.y, b.v.z); S.put(slot + 3, c.w.x, c.w.y, c.w.z, c.v.x); S.put(slot + 4, c.v.y, c.v.z, e0, e1);
}
LM_DEV void unstash_sv3(const Stash& S, int slot, SV& a, SV& b, SV& c) {
  float4 t0 = S.get(slot), t1 = S.get(slot + 1), t2 = S.get(slot + 2), t3 = S.get(slot + 3), t4 = S.get(slot + 4);
  a = sv(v3(t0.x, t0.y, t0.z), v3(t0.w, t1.x, t1.y)); b = sv(v3(t1.z, t1.w, t2.x), v3(t2.y, t2.z, t2.w)); c = sv(v3(t3.x, t3.y, t3.z), v3(t3.w, t4.x, t4.y));
}

// The pass-invariant terms of a sub-step, in the register layout the pass reads them in.  substep() computes them, writes them to the stash and
// runs the FIRST pass on the registers it has just computed; only a second pass (the active-set re-solve) reloads them from the stash, after the
// contact iterations - keeping them in registers across those would spill.  Until round 5 the first pass reloaded them too: 19 ds_read_b128
// behind 19 ds_write_b128 per sub-step, for values that were in registers (-DLM_PASS0_STASH: that form, tools/ab_build.py; substep<..., REG0 = 0>:
// that form for one kernel - k_step_w2 and the persistent rollouts, whose scratch grows with the register form: DESIGN.md 5.1).
#if defined(LM_PASS0_STASH) || defined(LM_WAVES2)      // (two wavefronts per SIMD: 256 registers have no room for the register form, see REG0)
#define LM_PASS0_REG 0
#else
#define LM_PASS0_REG 1
#endif
struct PassTerms {
  S6 Fq0, Fq1, Fq2;        // coupling columns
  float Ha[6], hq[3];      // limb joint-space inertia [00,01,02,11,12,22] and bias
  float Jq0[3]; f2 j12[3]; // tip velocity per unit joint rate, contact coordinates: row 0, rows (1 | 2)
  R4 PB[6];                // p = (fcs[i] | Jb0[i]) or (up_free[i] | Tp0[i]),  q = (row 1 | row 2)
  SI Isc;                  // limb composite inertia (MODE 0 only)
};
LM_DEV S6 s6(SV a) { S6 r; r.a = mk2(a.w.x, a.w.y); r.b = mk2(a.w.z, a.v.x); r.c = mk2(a.v.y, a.v.z); return r; }
// (a macro on substep()'s own locals: as a function taking the SVs by reference, the pair (b.w.x | r0.w.x) is formed by a two-float load from b
// before b is inlined, and b then stays in memory)
#define LM_PASS_ROWS(I, b, r0, r1, r2) { \
  I.PB[0].p = mk2(b.w.x, r0.w.x); I.PB[1].p = mk2(b.w.y, r0.w.y); I.PB[2].p = mk2(b.w.z, r0.w.z); \
  I.PB[3].p = mk2(b.v.x, r0.v.x); I.PB[4].p = mk2(b.v.y, r0.v.y); I.PB[5].p = mk2(b.v.z, r0.v.z); \
  I.PB[0].q = mk2(r1.w.x, r2.w.x); I.PB[1].q = mk2(r1.w.y, r2.w.y); I.PB[2].q = mk2(r1.w.z, r2.w.z); \
  I.PB[3].q = mk2(r1.v.x, r2.v.x); I.PB[4].q = mk2(r1.v.y, r2.v.y); I.PB[5].q = mk2(r1.v.z, r2.v.z); }
// The terms as the stash would hand them back: values in registers that the optimiser cannot see through, so that no expression of the pass is
// contracted with the expression that produced one of its inputs.  The first pass then rounds exactly as a pass fed from the stash (costs no instruction)
LM_DEV void pin(float& x) { asm("" : "+v"(x)); }
LM_DEV void pin(f2& x) { asm("" : "+v"(x)); }
LM_DEV void pin(S6& x) { pin(x.a); pin(x.b); pin(x.c); }
template <int MODE> LM_DEV void pin_terms(PassTerms& I) {
  // (no loops over the members: an index that is a variable until the loop is unrolled keeps the whole struct in memory too long)
  pin(I.Fq0); pin(I.Fq1); pin(I.Fq2);
  pin(I.Ha[0]); pin(I.Ha[1]); pin(I.Ha[2]); pin(I.Ha[3]); pin(I.Ha[4]); pin(I.Ha[5]);
  pin(I.hq[0]); pin(I.hq[1]); pin(I.hq[2]); pin(I.Jq0[0]); pin(I.Jq0[1]); pin(I.Jq0[2]); pin(I.j12[0]); pin(I.j12[1]); pin(I.j12[2]);
  pin(I.PB[0].p); pin(I.PB[1].p); pin(I.PB[2].p); pin(I.PB[3].p); pin(I.PB[4].p); pin(I.PB[5].p);
  pin(I.PB[0].q); pin(I.PB[1].q); pin(I.PB[2].q); pin(I.PB[3].q); pin(I.PB[4].q); pin(I.PB[5].q);
  if (MODE == 0) { pin(I.Isc.m); pin(I.Isc.h.x); pin(I.Isc.h.y); pin(I.Isc.h.z); pin(I.Isc.xx); pin(I.Isc.yy); pin(I.Isc.zz); pin(I.Isc.xy); pin(I.Isc.xz); pin(I.Isc.yz); }
}
// Stash layout: slots 0-4 Fq0..2 (LM_WAVES2: Isc.xz, Isc.yz ride in the free half of slot 4), 5-6 H and hq[0..1], 7 (hq[2] | Jq row 0), 8-9 Jq rows
// (1 | 2), 10-12 PB[i].p, 13-15 PB[i].q, MODE 0: 16-18 Isc
LM_DEV void put2(const Stash& St, int slot, f2 a, f2 b) { St.put(slot, a.x, a.y, b.x, b.y); }
template <int MODE> LM_DEV void stash_terms(const Stash& St, const PassTerms& I) {
  put2(St, 0, I.Fq0.a, I.Fq0.b); put2(St, 1, I.Fq0.c, I.Fq1.a); put2(St, 2, I.Fq1.b, I.Fq1.c); put2(St, 3, I.Fq2.a, I.Fq2.b);
#ifdef LM_WAVES2
  St.put(4, I.Fq2.c.x, I.Fq2.c.y, I.Isc.xz, I.Isc.yz);
#else
  St.put(4, I.Fq2.c.x, I.Fq2.c.y, 0.f, 0.f);
#endif
  St.put(5, I.Ha[0], I.Ha[1], I.Ha[2], I.Ha[3]); St.put(6, I.Ha[4], I.Ha[5], I.hq[0], I.hq[1]);
  St.put(7, I.hq[2], I.Jq0[0], I.Jq0[1], I.Jq0[2]);
  put2(St, 8, I.j12[0], I.j12[1]); put2(St, 9, I.j12[2], sp2(0.f));
  put2(St, 10, I.PB[0].p, I.PB[1].p); put2(St, 11, I.PB[2].p, I.PB[3].p); put2(St, 12, I.PB[4].p, I.PB[5].p);
  put2(St, 13, I.PB[0].q, I.PB[1].q); put2(St, 14, I.PB[2].q, I.PB[3].q); put2(St, 15, I.PB[4].q, I.PB[5].q);
  if (MODE == 0) {
    St.put(16, I.Isc.m, I.Isc.h.x, I.Isc.h.y, I.Isc.h.z); St.put(17, I.Isc.xx, I.Isc.yy, I.Isc.zz, I.Isc.xy);
#ifndef LM_WAVES2
    St.put(18, I.Isc.xz, I.Isc.yz, 0.f, 0.f);
#endif
  }
}
#ifdef LM_HELPER_WAVE
// k_step_h3's wavefront 0 computes, pins and stashes the inertia chain's terms only (MODE 0: slots 0-6 with hq zero, 16-18); slots 7-15 are
// written by the terms helper (helper_wave_terms)
LM_DEV void pin_chain(PassTerms& I) {
  pin(I.Fq0); pin(I.Fq1); pin(I.Fq2);
  pin(I.Ha[0]); pin(I.Ha[1]); pin(I.Ha[2]); pin(I.Ha[3]); pin(I.Ha[4]); pin(I.Ha[5]);
  pin(I.Isc.m); pin(I.Isc.h.x); pin(I.Isc.h.y); pin(I.Isc.h.z); pin(I.Isc.xx); pin(I.Isc.yy); pin(I.Isc.zz); pin(I.Isc.xy); pin(I.Isc.xz); pin(I.Isc.yz);
}
LM_DEV void stash_chain(const Stash& St, const PassTerms& I) {
  put2(St, 0, I.Fq0.a, I.Fq0.b); put2(St, 1, I.Fq0.c, I.Fq1.a); put2(St, 2, I.Fq1.b, I.Fq1.c); put2(St, 3, I.Fq2.a, I.Fq2.b);
  St.put(4, I.Fq2.c.x, I.Fq2.c.y, 0.f, 0.f);
  St.put(5, I.Ha[0], I.Ha[1], I.Ha[2], I.Ha[3]); St.put(6, I.Ha[4], I.Ha[5], 0.f, 0.f);
  St.put(16, I.Isc.m, I.Isc.h.x, I.Isc.h.y, I.Isc.h.z); St.put(17, I.Isc.xx, I.Isc.yy, I.Isc.zz, I.Isc.xy); St.put(18, I.Isc.xz, I.Isc.yz, 0.f, 0.f);
}
#endif
template <int MODE> LM_DEV void unstash_terms(const Stash& St, PassTerms& I) {
  asm volatile("" ::: "memory");          // keep the stash reloads where the pass that needs them starts (no hoisting across the PGS loop)
  float isc_xz = 0.f, isc_yz = 0.f;
  {
    const float4 t0 = St.get(0), t1 = St.get(1), t2 = St.get(2), t3 = St.get(3), t4 = St.get(4);
    isc_xz = t4.z; isc_yz = t4.w;
    I.Fq0.a = mk2(t0.x, t0.y); I.Fq0.b = mk2(t0.z, t0.w); I.Fq0.c = mk2(t1.x, t1.y);
    I.Fq1.a = mk2(t1.z, t1.w); I.Fq1.b = mk2(t2.x, t2.y); I.Fq1.c = mk2(t2.z, t2.w);
    I.Fq2.a = mk2(t3.x, t3.y); I.Fq2.b = mk2(t3.z, t3.w); I.Fq2.c = mk2(t4.x, t4.y);
  }
  const float4 h5 = St.get(5), h6 = St.get(6), h7 = St.get(7), h8 = St.get(8), h9 = St.get(9);
  I.Ha[0] = h5.x; I.Ha[1] = h5.y; I.Ha[2] = h5.z; I.Ha[3] = h5.w; I.Ha[4] = h6.x; I.Ha[5] = h6.y;
  I.hq[0] = h6.z; I.hq[1] = h6.w; I.hq[2] = h7.x;
  I.Jq0[0] = h7.y; I.Jq0[1] = h7.z; I.Jq0[2] = h7.w;
  I.j12[0] = mk2(h8.x, h8.y); I.j12[1] = mk2(h8.z, h8.w); I.j12[2] = mk2(h9.x, h9.y);
  {
    const float4 g0 = St.get(10), g1 = St.get(11), g2 = St.get(12), g3 = St.get(13), g4 = St.get(14), g5 = St.get(15);
    I.PB[0].p = mk2(g0.x, g0.y); I.PB[1].p = mk2(g0.z, g0.w); I.PB[2].p = mk2(g1.x, g1.y); I.PB[3].p = mk2(g1.z, g1.w); I.PB[4].p = mk2(g2.x, g2.y); I.PB[5].p = mk2(g2.z, g2.w);
    I.PB[0].q = mk2(g3.x, g3.y); I.PB[1].q = mk2(g3.z, g3.w); I.PB[2].q = mk2(g4.x, g4.y); I.PB[3].q = mk2(g4.z, g4.w); I.PB[4].q = mk2(g5.x, g5.y); I.PB[5].q = mk2(g5.z, g5.w);
  }
  if (MODE == 0) {
#ifdef LM_WAVES2
    const float4 g16 = St.get(16), g17 = St.get(17), g18 = make_float4(isc_xz, isc_yz, 0.f, 0.f);
#else
    const float4 g16 = St.get(16), g17 = St.get(17), g18 = St.get(18); (void)isc_xz; (void)isc_yz;
#endif
    I.Isc.m = g16.x; I.Isc.h = v3(g16.y, g16.z, g16.w); I.Isc.xx = g17.x; I.Isc.yy = g17.y; I.Isc.zz = g17.z; I.Isc.xy = g17.w; I.Isc.xz = g18.x; I.Isc.yz = g18.y;
  }
}

// Per-env plate inertia of the randomised kernels (mass channels): the plate's inertia about its COM is diagonal, so the inverse of its spatial
// inertia about the plate origin is  X^-1 diag(1 / I_com, 1 / m) X^-T  with X the shift by the COM: seven numbers instead of a 6 x 6 matrix.
// For a wrench (n about the origin, f):  alpha = (n - c x f) / I_com,  a_origin = f / m + c x alpha
template <class T> struct PlateInvT { V3T<T> ii, c; T im; };
LM_DEV PlateInvT<float> plate_inv(const lm_params* __restrict__ P, float m, float s) {
  PlateInvT<float> Q; Q.ii = v3(1.0f / (s * P->plate_inertia[0]), 1.0f / (s * P->plate_inertia[1]), 1.0f / (s * P->plate_inertia[2]));
  Q.c = v3(P->plate_com[0], P->plate_com[1], P->plate_com[2]); Q.im = 1.0f / m; return Q;
}
template <class T> LM_DEV void plate_inv_apply(const PlateInvT<T>& Q, V3T<T> n, V3T<T> f, V3T<T>& al, V3T<T>& a) {
  const V3T<T> nc = n - cross(Q.c, f);
  al = v3t<T>(nc.x * Q.ii.x, nc.y * Q.ii.y, nc.z * Q.ii.z);
  a = fma3(Q.im, f, cross(Q.c, al));
}
LM_DEV SI plate_inertia_env(const lm_params* __restrict__ P, float m, float s) {      // spatial inertia about the plate origin from (m, COM, s x I_com)
  const V3 c = v3(P->plate_com[0], P->plate_com[1], P->plate_com[2]); const float cc = dot(c, c);
  SI I; I.m = m; I.h = m * c;
  I.xx = fmaf(m, cc - c.x * c.x, s * P->plate_inertia[0]); I.yy = fmaf(m, cc - c.y * c.y, s * P->plate_inertia[1]); I.zz = fmaf(m, cc - c.z * c.z, s * P->plate_inertia[2]);
  I.xy = -m * c.x * c.y; I.xz = -m * c.x * c.z; I.yz = -m * c.y * c.z;
  return I;
}

// One drive pass of a sub-step: the limb's joints eliminated against the given drive state (sat / tsat), the hub or plate solve, the contact
// operator and the PGS, on the pass-invariant terms I - the registers substep() has just computed (first pass) or the stash's copy (second pass).
// Out: the joint rates qdn and the free body's velocity un after the pass, and (CF) the contact impulses lamc.
// HW 1 (the first pass of wavefront 0 of k_step_h2): I.hq and the bias halves PB[i].p.x are not in I; the pass fetches them from the helper
// wavefront's slots (Hd) behind its second barrier, which stands where they are first needed - after the articulated hub inertia, so that
// wavefront 0 has more work before the barrier than the helper has and does not wait there.
// HW 2 (the first pass of wavefront 0 of k_step_h3): as HW 1, and Jq, the hub rows PB[i].p.y / PB[i].q and bn are not in I / bn either; the pass
// reads them behind the same barrier from stash slots 7-15, where the terms helper (helper_wave_terms) has written them.
// Row I of the pass's four-vector elimination, on the names of the function it stands in (cp, j12, PB, K0..K2, T, X); BIAS: what the hub solve
// takes for the bias column.  A macro, so that substep_pass and the helpers of k_step_h3 (helper_xblocks) compile the same lines
#define LM_PROW(I, BIAS) { \
      const f2 k0 = sp2(comp<I>(K0)), k1 = sp2(comp<I>(K1)), k2 = sp2(comp<I>(K2)); \
      T[I].p = fma_(cp[2], k2, fma_(cp[1], k1, fma_(cp[0], k0, PB[I].p))); \
      T[I].q = fma_(-j12[2], k2, fma_(-j12[1], k1, fma_(-j12[0], k0, PB[I].q))); \
      X[I].p = mk2(BIAS, T[I].p.y); X[I].q = T[I].q; }
template <int MODE, int VAR, int DR, int CF, int HW = 0>
LM_DEV void substep_pass(const lm_params* __restrict__ P, int limb, const FreeBody& F, const PassTerms& I, float dt, float kd, const float cjv[3],
                         const bool sat[3], const float tsat[3], const float tgt[3], const float qd[3], float bn, float mu_dr,
                         bool mp_on, float m_plate, float s_plate, float qdn[3], SV& un, float lamc[3], const Stash* Hd = nullptr) {
  const S6 Fq0 = I.Fq0, Fq1 = I.Fq1, Fq2 = I.Fq2;
  float Ha[6] = {I.Ha[0], I.Ha[1], I.Ha[2], I.Ha[3], I.Ha[4], I.Ha[5]}, r[3];
  const float hq[3] = {I.hq[0], I.hq[1], I.hq[2]};
  R4 PBh[6];      // HW: the rows with the helper's bias wrench
  const float Jq_[3][3] = {{I.Jq0[0], I.Jq0[1], I.Jq0[2]}, {I.j12[0].x, I.j12[1].x, I.j12[2].x}, {I.j12[0].y, I.j12[1].y, I.j12[2].y}};
  const f2 j12_[3] = {I.j12[0], I.j12[1], I.j12[2]};      // (Jq[1][c] | Jq[2][c])
  float Jqh[3][3]; f2 j12h[3]; float bnh = bn;      // HW 2: the terms helper's, fetched behind the barrier
  const float (*Jq)[3] = HW == 2 ? Jqh : Jq_;
  const f2* j12 = HW == 2 ? j12h : j12_;
  const R4* PB = HW ? PBh : I.PB;
  const int di[3] = {0, 3, 5};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float cj = cjv[a];
    {
      // The drive terms, with their rounding written out: dt x (the damping that applies) is fused into H's diagonal, the unsaturated drive
      // torque kd (q*' - q') and the damping torque cj q' are rounded products, then two subtractions.  That is how the compiler contracted
      // `Ha += sat ? dt cj : dt (kd + cj);  r = (sat ? tsat : kd (tgt - qd)) - cj qd - hq` while every pass sat in one loop; left to it, a pass that
      // knows more about sat[] (the first pass on registers) is contracted differently from one that does not (k_step_w2, the persistent
      // rollouts), and the kernels must agree bit for bit
#pragma clang fp contract(off)
      Ha[di[a]] = fmaf(dt, sat[a] ? cj : kd + cj, Ha[di[a]]);                  // viscous joint damping is implicit in both cases
      const float rr = sat[a] ? tsat[a] : kd * (tgt[a] - qd[a]);
      const float damp = cj * qd[a];
      r[a] = HW ? rr - damp : (rr - damp) - hq[a];      // (HW: the joint-space bias is subtracted behind the barrier)
    }
  }
  float Hi[6]; inv3sym(Ha, Hi);
  // K = Fq Hinv  (columns)
  const S6 K0 = fma6(Hi[0], Fq0, fma6(Hi[1], Fq1, Hi[2] * Fq2));
  const S6 K1 = fma6(Hi[1], Fq0, fma6(Hi[3], Fq1, Hi[4] * Fq2));
  const S6 K2 = fma6(Hi[2], Fq0, fma6(Hi[4], Fq1, Hi[5] * Fq2));
  float qdd[3], qdf[3], v0f[6], vf[3];
  R4 T[6], X[6];
  if (MODE == 0) {
    // articulated hub inertia  A = sum over the quad of (Isc - K F^T): rows of pairs, upper triangle only
    float A0[6][6]; si_to_66(I.Isc, A0);
    float A[6][6];
#define LM_AROW(I) { \
      const f2 k0 = sp2(comp<I>(K0)), k1 = sp2(comp<I>(K1)), k2 = sp2(comp<I>(K2)); \
      _Pragma("unroll") for (int jp = (I) / 2; jp < 3; jp++) { \
        const f2 f0 = jp == 0 ? Fq0.a : jp == 1 ? Fq0.b : Fq0.c, f1 = jp == 0 ? Fq1.a : jp == 1 ? Fq1.b : Fq1.c, f2_ = jp == 0 ? Fq2.a : jp == 1 ? Fq2.b : Fq2.c; \
        const f2 v = fma_(-k2, f2_, fma_(-k1, f1, fma_(-k0, f0, mk2(A0[I][2 * jp], A0[I][2 * jp + 1])))); \
        if (2 * jp >= (I)) A[I][2 * jp] = quad_sum(v.x); \
        A[I][2 * jp + 1] = quad_sum(v.y); } }
    LM_AROW(0) LM_AROW(1) LM_AROW(2) LM_AROW(3) LM_AROW(4) LM_AROW(5)
#undef LM_AROW
    Chol6 Ch;
#ifdef LM_HELPER_WAVE
    if (HW) {
#if LM_HELPER_WAVE >= 2 && LM_H3_XBLOCKS
      if (HW == 2) {
        // k_step_h3: the factor in front of the barrier (its input is this wavefront's own), and what the helpers need for the cross blocks
        // (helper_xblocks) with it: whole rounded results that the lines below only use as operands
        chol6(A, Ch);
        put2(*Hd, XB_IN_A, K0.a, K0.b); put2(*Hd, XB_IN_A + 1, K0.c, K1.a); put2(*Hd, XB_IN_A + 2, K1.b, K1.c); put2(*Hd, XB_IN_A + 3, K2.a, K2.b);
        Hd->put(XB_IN_A + 4, K2.c.x, K2.c.y, Ch.d[0], Ch.d[1]); Hd->put(XB_IN_B, Ch.d[2], Ch.d[3], Ch.d[4], Ch.d[5]);
        Hd->put(XB_IN_B + 1, Ch.L[1][0], Ch.L[2][0], Ch.L[2][1], Ch.L[3][0]); Hd->put(XB_IN_B + 2, Ch.L[3][1], Ch.L[3][2], Ch.L[4][0], Ch.L[4][1]);
        Hd->put(XB_IN_B + 3, Ch.L[4][2], Ch.L[4][3], Ch.L[5][0], Ch.L[5][1]); Hd->put(XB_IN_B + 4, Ch.L[5][2], Ch.L[5][3], Ch.L[5][4], 0.f);
      }
#endif
      hw_barrier();      // the helper's second barrier of the sub-step: its bias terms are in LDS
      const float4 b0 = Hd->get(HAND_OUT), b1 = Hd->get(HAND_OUT + 1), b2 = Hd->get(HAND_OUT + 2);
      const float fcs[6] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y}, hqh[3] = {b1.z, b1.w, b2.x};
      if (HW == 2) {
        // k_step_h3: the contact rows and the approach rate are the terms helper's (helper_wave_terms), in the stash slots the second pass
        // reads them from.  Read back from LDS they are what pin_terms made of them in k_step: values no expression is contracted with
        const float4 t7 = Hd->get(7), t8 = Hd->get(8), t9 = Hd->get(9);
        const float4 g0 = Hd->get(10), g1 = Hd->get(11), g2 = Hd->get(12), g3 = Hd->get(13), g4 = Hd->get(14), g5 = Hd->get(15);
        j12h[0] = mk2(t8.x, t8.y); j12h[1] = mk2(t8.z, t8.w); j12h[2] = mk2(t9.x, t9.y); bnh = t9.z;
        Jqh[0][0] = t7.y; Jqh[0][1] = t7.z; Jqh[0][2] = t7.w;
#pragma unroll
        for (int c = 0; c < 3; c++) { Jqh[1][c] = j12h[c].x; Jqh[2][c] = j12h[c].y; }
        PBh[0].p = mk2(fcs[0], g0.y); PBh[1].p = mk2(fcs[1], g0.w); PBh[2].p = mk2(fcs[2], g1.y);
        PBh[3].p = mk2(fcs[3], g1.w); PBh[4].p = mk2(fcs[4], g2.y); PBh[5].p = mk2(fcs[5], g2.w);
        PBh[0].q = mk2(g3.x, g3.y); PBh[1].q = mk2(g3.z, g3.w); PBh[2].q = mk2(g4.x, g4.y);
        PBh[3].q = mk2(g4.z, g4.w); PBh[4].q = mk2(g5.x, g5.y); PBh[5].q = mk2(g5.z, g5.w);
      } else {
#pragma unroll
      for (int i = 0; i < 6; i++) { PBh[i].p = mk2(fcs[i], I.PB[i].p.y); PBh[i].q = I.PB[i].q; }
      }
#pragma unroll
      for (int a = 0; a < 3; a++) {
#pragma clang fp contract(off)
        r[a] = r[a] - hqh[a];
      }
    }
#endif
    if (!(HW == 2 && LM_H3_XBLOCKS)) chol6(A, Ch);
    // (bias | row 0) and (row 1 | row 2) with the limb's joints eliminated:  P = PB + coefficient x K,  T_r = Jb_r - K Jq_r^T
    const f2 cp[3] = {mk2(r[0], -Jq[0][0]), mk2(r[1], -Jq[0][1]), mk2(r[2], -Jq[0][2])};
    LM_PROW(0, -quad_sum(T[0].p.x)) LM_PROW(1, -quad_sum(T[1].p.x)) LM_PROW(2, -quad_sum(T[2].p.x))
    LM_PROW(3, -quad_sum(T[3].p.x)) LM_PROW(4, -quad_sum(T[4].p.x)) LM_PROW(5, -quad_sum(T[5].p.x))
    chol6_solve4(Ch, X);          // X = (a0 | B0), (B1 | B2): hub acceleration and Phi T without forming Phi
    float t0 = r[0], t1 = r[1], t2 = r[2];
#define LM_TROW(I) { const float a = X[I].p.x; t0 = fmaf(-comp<I>(Fq0), a, t0); t1 = fmaf(-comp<I>(Fq1), a, t1); t2 = fmaf(-comp<I>(Fq2), a, t2); }
    LM_TROW(0) LM_TROW(1) LM_TROW(2) LM_TROW(3) LM_TROW(4) LM_TROW(5)
#undef LM_TROW
    qdd[0] = Hi[0] * t0 + Hi[1] * t1 + Hi[2] * t2; qdd[1] = Hi[1] * t0 + Hi[3] * t1 + Hi[4] * t2; qdd[2] = Hi[2] * t0 + Hi[4] * t1 + Hi[5] * t2;
    const float u6[6] = {F.u.w.x, F.u.w.y, F.u.w.z, F.u.v.x, F.u.v.y, F.u.v.z};
#pragma unroll
    for (int i = 0; i < 6; i++) v0f[i] = fmaf(dt, X[i].p.x, u6[i]);
  } else {
    qdd[0] = Hi[0] * r[0] + Hi[1] * r[1] + Hi[2] * r[2]; qdd[1] = Hi[1] * r[0] + Hi[3] * r[1] + Hi[4] * r[2]; qdd[2] = Hi[2] * r[0] + Hi[4] * r[1] + Hi[5] * r[2];
#pragma unroll
    for (int i = 0; i < 6; i++) { v0f[i] = PB[i].p.x; T[i] = PB[i]; }
    if (mp_on) {
      // B = Phi' T with this env's plate mass / inertia factor, through the COM (plate_inv_apply), both halves of the four-vector layout
      const PlateInvT<float> Q1 = plate_inv(P, m_plate, s_plate);
      PlateInvT<f2> Q; Q.ii = bc(Q1.ii); Q.c = bc(Q1.c); Q.im = sp2(Q1.im);
      V3P al, ac;
      plate_inv_apply<f2>(Q, v3(T[0].p, T[1].p, T[2].p), v3(T[3].p, T[4].p, T[5].p), al, ac);
      X[0].p = al.x; X[1].p = al.y; X[2].p = al.z; X[3].p = ac.x; X[4].p = ac.y; X[5].p = ac.z;
      plate_inv_apply<f2>(Q, v3(T[0].q, T[1].q, T[2].q), v3(T[3].q, T[4].q, T[5].q), al, ac);
      X[0].q = al.x; X[1].q = al.y; X[2].q = al.z; X[3].q = ac.x; X[4].q = ac.y; X[5].q = ac.z;
    } else {
    // B = Phi T with the plate's constant inverse inertia
#pragma unroll
    for (int i = 0; i < 6; i++) {
      f2 bp = sp2(0.f), bq = sp2(0.f);
#pragma unroll
      for (int j = 0; j < 6; j++) { const f2 ph = sp2(P->plate_phi[6 * i + j]); bp = fma_(ph, T[j].p, bp); bq = fma_(ph, T[j].q, bq); }
      X[i].p = bp; X[i].q = bq;
    }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) qdf[a] = fmaf(dt, qdd[a], qd[a]);
  // contact operator
  float Wl[6];
  float JH[3][3];   // Jq * Hinv
#pragma unroll
  for (int rr = 0; rr < 3; rr++) {
    JH[rr][0] = Jq[rr][0] * Hi[0] + Jq[rr][1] * Hi[1] + Jq[rr][2] * Hi[2];
    JH[rr][1] = Jq[rr][0] * Hi[1] + Jq[rr][1] * Hi[3] + Jq[rr][2] * Hi[4];
    JH[rr][2] = Jq[rr][0] * Hi[2] + Jq[rr][1] * Hi[4] + Jq[rr][2] * Hi[5];
  }
  Wl[0] = JH[0][0] * Jq[0][0] + JH[0][1] * Jq[0][1] + JH[0][2] * Jq[0][2];
  Wl[1] = JH[0][0] * Jq[1][0] + JH[0][1] * Jq[1][1] + JH[0][2] * Jq[1][2];
  Wl[2] = JH[0][0] * Jq[2][0] + JH[0][1] * Jq[2][1] + JH[0][2] * Jq[2][2];
  Wl[3] = JH[1][0] * Jq[1][0] + JH[1][1] * Jq[1][1] + JH[1][2] * Jq[1][2];
  Wl[4] = JH[1][0] * Jq[2][0] + JH[1][1] * Jq[2][1] + JH[1][2] * Jq[2][2];
  Wl[5] = JH[2][0] * Jq[2][0] + JH[2][1] * Jq[2][1] + JH[2][2] * Jq[2][2];
  // free contact-space velocity: hub / plate rows (before the joints were eliminated) on v0f, plus the joint part
  {
    float a = 0.f; f2 b = sp2(0.f);
#pragma unroll
    for (int i = 0; i < 6; i++) { a = fmaf(PB[i].p.y, v0f[i], a); b = fma_(PB[i].q, sp2(v0f[i]), b); }
    vf[0] = a + (Jq[0][0] * qdf[0] + Jq[0][1] * qdf[1] + Jq[0][2] * qdf[2]);
    vf[1] = b.x + (Jq[1][0] * qdf[0] + Jq[1][1] * qdf[1] + Jq[1][2] * qdf[2]);
    vf[2] = b.y + (Jq[2][0] * qdf[0] + Jq[2][1] * qdf[1] + Jq[2][2] * qdf[2]);
  }
  float lam[3], w[6];
  LM_STAMP(3);
  constexpr int XB = (HW == 2 && LM_H3_XBLOCKS) ? 1 : 0;
  const int iters = XB ? P->pgs_iters : 0;      // (XB: read in front of barrier B3, not behind it with the sweeps waiting for it)
  PgsState S; pgs_setup<XB>(S, limb, DR ? mu_dr : P->mu, HW == 2 ? bnh : bn, vf, Wl, T, X, Hd);
  pgs_sweeps(S, 0, XB ? iters : P->pgs_iters);
  pgs_finish(S, DR ? mu_dr : P->mu, X, lam, w);
  if (CF) { lamc[0] = lam[0]; lamc[1] = lam[1]; lamc[2] = lam[2]; }
  un = sv(v3(v0f[0] + w[0], v0f[1] + w[1], v0f[2] + w[2]), v3(v0f[3] + w[3], v0f[4] + w[4], v0f[5] + w[5]));
#pragma unroll
  for (int a = 0; a < 3; a++) qdn[a] = qdf[a] + JH[0][a] * lam[0] + JH[1][a] * lam[1] + JH[2][a] * lam[2];
  if (MODE == 0) {
#define LM_WROW(I) { qdn[0] = fmaf(-comp<I>(K0), w[I], qdn[0]); qdn[1] = fmaf(-comp<I>(K1), w[I], qdn[1]); qdn[2] = fmaf(-comp<I>(K2), w[I], qdn[2]); }
    LM_WROW(0) LM_WROW(1) LM_WROW(2) LM_WROW(3) LM_WROW(4) LM_WROW(5)
#undef LM_WROW
  }
  LM_STAMP(4);
}

#ifdef LM_HELPER_WAVE
#if LM_HELPER_WAVE >= 2
// wavefront 0 of k_step_h3 (pgs_setup, XB): barrier B3, then the four raw cross blocks from the helpers' hand-back slots
LM_DEV void xblocks_fetch(const Stash* Hd, XRaw& R0, XRaw& R1, XRaw& R2, XRaw& R3) {
#if LM_H3_XBLOCKS
  hw_barrier();      // B3: the cross blocks are in LDS
  const float4 a0 = Hd->get(XB_OUT), a1 = Hd->get(XB_OUT + 1), a2 = Hd->get(XB_OUT + 2), a3 = Hd->get(XB_OUT + 3), a4 = Hd->get(XB_OUT + 4);
  const float4 b0 = Hd->get(XB_OUT + 5), b1 = Hd->get(XB_OUT + 6), b2 = Hd->get(XB_OUT + 7), b3 = Hd->get(XB_OUT + 8), b4 = Hd->get(XB_OUT + 9);
  R0.a00 = a0.x; R0.a0t = mk2(a0.y, a0.z); R0.c0 = mk2(a0.w, a1.x); R0.c1 = mk2(a1.y, a1.z); R0.c2 = mk2(a1.w, a2.x);
  R1.a00 = a2.y; R1.a0t = mk2(a2.z, a2.w); R1.c0 = mk2(a3.x, a3.y); R1.c1 = mk2(a3.z, a3.w); R1.c2 = mk2(a4.x, a4.y);
  R2.a00 = b0.x; R2.a0t = mk2(b0.y, b0.z); R2.c0 = mk2(b0.w, b1.x); R2.c1 = mk2(b1.y, b1.z); R2.c2 = mk2(b1.w, b2.x);
  R3.a00 = b2.y; R3.a0t = mk2(b2.z, b2.w); R3.c0 = mk2(b3.x, b3.y); R3.c1 = mk2(b3.z, b3.w); R3.c2 = mk2(b4.x, b4.y);
#endif
}
#if LM_H3_XBLOCKS
// The cross blocks of the contact operator on the two helpers of k_step_h3 (LM_H3_XBLOCKS).  Behind the second barrier of a
// sub-step wavefront 0 still eliminates, solves and builds its own block alone, about 700 instructions before the first PGS turn, while the
// helpers wait for the next sub-step.  Here each helper takes K and the hub factor (wavefront 0 factors in front of that barrier and publishes
// both, XB_IN_*) and the contact rows (slots 7-15, the terms helper's), runs the pass's elimination (LM_PROW) and hub solve (chol6_solve4) on
// the three contact columns - the bias column, the .p.x half, is zero here and is wavefront 0's alone - and then two of the four raw blocks
// (pgs_cross_raw<KA>, <KB>) into its five hand-back slots, and passes barrier B3; wavefront 0 passes B3 where pgs_setup needs the blocks.
// Same bits as k_step: every line up to the blocks is an explicit fma on rounded operands (nothing for the compiler to contract another way),
// the two halves of a packed instruction do not see each other, and the blocks cross the cut raw, before the own-block select and the scaling.
// B3 follows the discipline written above helper_wave: once per sub-step in straight-line code in all three wavefronts; the second pass (HW 0)
// computes its own blocks and has no barrier.  Hazards: wavefront 0 writes the hand-in slots behind the sub-step's first barrier, the helpers
// read them between the second and B3; the helpers write the hand-back slots behind the second barrier, wavefront 0 reads them behind B3 and
// has used them before the next sub-step's first.
template <int KA, int KB>
LM_DEV void helper_xblocks(const Stash& St, int out) {
  const float4 i0 = St.get(XB_IN_A), i1 = St.get(XB_IN_A + 1), i2 = St.get(XB_IN_A + 2), i3 = St.get(XB_IN_A + 3), i4 = St.get(XB_IN_A + 4);
  const float4 i5 = St.get(XB_IN_B), i6 = St.get(XB_IN_B + 1), i7 = St.get(XB_IN_B + 2), i8 = St.get(XB_IN_B + 3), i9 = St.get(XB_IN_B + 4);
  const float4 t7 = St.get(7), t8 = St.get(8), t9 = St.get(9);
  const float4 g0 = St.get(10), g1 = St.get(11), g2 = St.get(12), g3 = St.get(13), g4 = St.get(14), g5 = St.get(15);
  S6 K0, K1, K2;
  K0.a = mk2(i0.x, i0.y); K0.b = mk2(i0.z, i0.w); K0.c = mk2(i1.x, i1.y); K1.a = mk2(i1.z, i1.w); K1.b = mk2(i2.x, i2.y); K1.c = mk2(i2.z, i2.w);
  K2.a = mk2(i3.x, i3.y); K2.b = mk2(i3.z, i3.w); K2.c = mk2(i4.x, i4.y);
  Chol6 Ch;      // (the strictly lower triangle and d: all the solve reads)
  Ch.d[0] = i4.z; Ch.d[1] = i4.w; Ch.d[2] = i5.x; Ch.d[3] = i5.y; Ch.d[4] = i5.z; Ch.d[5] = i5.w;
  Ch.L[1][0] = i6.x; Ch.L[2][0] = i6.y; Ch.L[2][1] = i6.z; Ch.L[3][0] = i6.w; Ch.L[3][1] = i7.x; Ch.L[3][2] = i7.y; Ch.L[4][0] = i7.z; Ch.L[4][1] = i7.w;
  Ch.L[4][2] = i8.x; Ch.L[4][3] = i8.y; Ch.L[5][0] = i8.z; Ch.L[5][1] = i8.w; Ch.L[5][2] = i9.x; Ch.L[5][3] = i9.y; Ch.L[5][4] = i9.z;
  const f2 cp[3] = {mk2(0.f, -t7.y), mk2(0.f, -t7.z), mk2(0.f, -t7.w)};
  const f2 j12[3] = {mk2(t8.x, t8.y), mk2(t8.z, t8.w), mk2(t9.x, t9.y)};
  R4 PB[6], T[6], X[6];
  PB[0].p = mk2(0.f, g0.y); PB[1].p = mk2(0.f, g0.w); PB[2].p = mk2(0.f, g1.y); PB[3].p = mk2(0.f, g1.w); PB[4].p = mk2(0.f, g2.y); PB[5].p = mk2(0.f, g2.w);
  PB[0].q = mk2(g3.x, g3.y); PB[1].q = mk2(g3.z, g3.w); PB[2].q = mk2(g4.x, g4.y); PB[3].q = mk2(g4.z, g4.w); PB[4].q = mk2(g5.x, g5.y); PB[5].q = mk2(g5.z, g5.w);
  LM_PROW(0, 0.f) LM_PROW(1, 0.f) LM_PROW(2, 0.f) LM_PROW(3, 0.f) LM_PROW(4, 0.f) LM_PROW(5, 0.f)
  chol6_solve4(Ch, X);
  XRaw A, B; pgs_cross_raw<KA>(T, X, A); pgs_cross_raw<KB>(T, X, B);
  St.put(out, A.a00, A.a0t.x, A.a0t.y, A.c0.x); St.put(out + 1, A.c0.y, A.c1.x, A.c1.y, A.c2.x); St.put(out + 2, A.c2.y, B.a00, B.a0t.x, B.a0t.y);
  St.put(out + 3, B.c0.x, B.c0.y, B.c1.x, B.c1.y); St.put(out + 4, B.c2.x, B.c2.y, 0.f, 0.f);
}
#endif
#endif
// The helper wavefront of k_step_h2 (threads 64-127; lane l serves lane l of wavefront 0).  Per locomotion sub-step it recomputes the limb
// kinematics and the placed inertias from the joint state wavefront 0 published, runs the bias chain of limb_dynamics and the hub's own bias
// term (limb 0 carries the hub, as in substep) and leaves the limb's bias wrench and joint-space bias for wavefront 0: about 900 instructions
// that wavefront 0, which is bound by its own instruction stream, no longer issues.  It reads the table in LDS and the parameter block, and
// touches no other memory.
//
// Same bits as k_step: the helper's inputs are values that k_step, too, holds rounded in registers at the top of a sub-step (loop-carried
// state, or products that only feed further products), its outputs are values that k_step pins before the pass reads them (pin_terms), and
// in between both kernels compile the same lines.  No expression straddles the cut in a way the compiler could contract differently: the only
// sums of two products that meet across it are the components of Ic.h = I41.h + I32.h, where the product with fewer uses is fused, and that is
// I41.h with and without the bias chain (I32 also feeds Fp).  The fictitious acceleration is handed over as row 2 of the base's rotation, not
// as gravity x that row, because k_step fuses that product into the shell's acceleration.
//
// Barriers: two per sub-step in each wavefront, in straight-line code outside every branch of the sub-step (second pass, reset, lane
// divergence); both wavefronts take nsub from the same kernel argument or the same word of the parameter block, so they arrive the same number
// of times.  Inactive lanes of a ragged wavefront run along.  No flag in memory is polled anywhere.  A wavefront that has ended no longer counts
// at a barrier, so a helper that returns at once (manipulation block, nsub = 0) cannot hold wavefront 0 up, and a mismatch could not hang: it
// would show as wrong bits (tests/test_gpu_helper_wave.py).
// Hazards: the helper reads HAND_IN between the barriers and wavefront 0 writes it before the first; wavefront 0 reads HAND_OUT after the second
// and has its data (lgkmcnt(0)) before the next sub-step's first barrier, behind which the helper writes it again.
LM_DEV void helper_wave(const lm_params* __restrict__ P, const float* sTab, float4* sStash, int lane, int nsub) {
  const int limb = lane & 3;
  const float* th = sTab; const float* tl = sTab + HUB_FLOATS + limb * LIMB_STRIDE;
  Stash St; St.base = sStash; St.lane = lane;
  const float gravity = P->gravity;
  for (int s = 0; s < nsub; s++) {
    hw_barrier();      // the joint state of this sub-step is published (first sub-step: and the table committed)
    const float4 h0 = St.get(HAND_IN), h1 = St.get(HAND_IN + 1), h2 = St.get(HAND_IN + 2), h3 = St.get(HAND_IN + 3);
    const float q[3] = {h0.x, h0.y, h0.z}, qd[3] = {h0.w, h1.x, h1.y};
    const SV v0 = sv(v3(h1.z, h1.w, h2.x), v3(h2.y, h2.z, h2.w));
    const SV avp0 = sv(v3(0, 0, 0), gravity * v3(h3.x, h3.y, h3.z));      // fictitious acceleration = -gravity
    LimbKin K; limb_kinematics(tl, q, qd, K);
    LimbDyn D; limb_dynamics<0, 2>(tl, K, qd, v0, avp0, D);
    {
      // the hub's own bias term, as in substep()
      const float m0 = (limb == 0) ? 1.f : 0.f;
      SI I0 = hub_inertia(th);
      I0.m *= m0; I0.h = m0 * I0.h; I0.xx *= m0; I0.yy *= m0; I0.zz *= m0; I0.xy *= m0; I0.xz *= m0; I0.yz *= m0;
      D.fcs = D.fcs + I0 * avp0 + fcross(v0, I0 * v0);
    }
    St.put(HAND_OUT, D.fcs.w.x, D.fcs.w.y, D.fcs.w.z, D.fcs.v.x); St.put(HAND_OUT + 1, D.fcs.v.y, D.fcs.v.z, D.hq[0], D.hq[1]); St.put(HAND_OUT + 2, D.hq[2], 0.f, 0.f, 0.f);
    hw_barrier();      // the bias terms are in LDS
#if LM_HELPER_WAVE >= 2 && LM_H3_XBLOCKS
    helper_xblocks<2, 3>(St, XB_OUT + 5);
    hw_barrier();      // B3: the cross blocks are in LDS
#endif
  }
}
#if LM_HELPER_WAVE >= 2
// The terms helper of k_step_h3 (threads 128-191; lane l serves lane l of wavefront 0), a third wavefront on a third SIMD.  Between the same
// two barriers as helper_wave it recomputes the limb kinematics, takes the foot selects of limb_dynamics<0, 1> (its inertia chain is dead here
// and compiled away) and runs the locomotion branch of substep()'s contact geometry: the contact axes, the gap and the approach rate bn, the
// nine Jq dots and the three hub rows - the lines substep() compiles, on inputs that k_step holds rounded in registers too (row 2 of the
// base's rotation is only ever a factor, the base height is loop-carried state).  It writes them where stash_terms puts them, slots 7-15 with
// the bias halves zero as wavefront 0 of k_step_h2 leaves them, and bn in the spare half of slot 9.  Wavefront 0 reads the slots behind the
// second barrier (substep_pass, HW 2) and a second pass reads them again (unstash_terms); this wavefront writes them again only behind the
// next sub-step's first barrier, which wavefront 0 reaches with its LDS reads complete.  Same barrier discipline as helper_wave.
LM_DEV void helper_wave_terms(const lm_params* __restrict__ P, const float* sTab, float4* sStash, int lane, int nsub) {
  const int limb = lane & 3;
  const float* tl = sTab + HUB_FLOATS + limb * LIMB_STRIDE;
  Stash St; St.base = sStash; St.lane = lane;
  const float dt = P->dt, baumgarte = P->baumgarte, max_depen_vel = P->max_depen_vel;
  for (int s = 0; s < nsub; s++) {
    hw_barrier();      // the joint state of this sub-step is published
    const float4 h0 = St.get(HAND_IN), h1 = St.get(HAND_IN + 1), h2 = St.get(HAND_IN + 2), h3 = St.get(HAND_IN + 3);
    const float q[3] = {h0.x, h0.y, h0.z}, qd[3] = {h0.w, h1.x, h1.y};
    const SV v0 = sv(v3(h1.z, h1.w, h2.x), v3(h2.y, h2.z, h2.w));
    const SV avp0 = sv(v3(0, 0, 0), v3(0, 0, 0));      // (feeds the bias chain only)
    LimbKin K; limb_kinematics(tl, q, qd, K);
    LimbDyn D; limb_dynamics<0, 1>(tl, K, qd, v0, avp0, D);
    // ---- contact geometry of this limb's tip, as in substep() (MODE 0)
    V3 C0, C1, C2; float phi;
    C0 = v3(h3.x, h3.y, h3.z);
    C1 = rsqrtf(fmaxf(1.0f - C0.x * C0.x, 1.0e-12f)) * v3(1.0f - C0.x * C0.x, -C0.x * C0.y, -C0.x * C0.z);
    C2 = cross(C0, C1);
    phi = h3.w + dot(C0, D.x) - P->tip_radius;
    D.x = fma3(-P->tip_radius, C0, D.x);
    const float bn = (phi >= 0.f) ? phi / dt : fmaxf(baumgarte * phi / dt, -max_depen_vel);
    V3 e0 = K.s1.v + cross(K.s1.w, D.x);
    V3 e1 = D.j31.v + cross(D.j31.w, D.x);
    V3 e2 = D.j32.v + cross(D.j32.w, D.x);
    St.put(7, 0.f, dot(C0, e0), dot(C0, e1), dot(C0, e2));
    St.put(8, dot(C1, e0), dot(C2, e0), dot(C1, e1), dot(C2, e1)); St.put(9, dot(C1, e2), dot(C2, e2), bn, 0.f);
    const V3 n0 = cross(D.x, C0), n1 = cross(D.x, C1), n2 = cross(D.x, C2);
    St.put(10, 0.f, n0.x, 0.f, n0.y); St.put(11, 0.f, n0.z, 0.f, C0.x); St.put(12, 0.f, C0.y, 0.f, C0.z);
    St.put(13, n1.x, n2.x, n1.y, n2.y); St.put(14, n1.z, n2.z, C1.x, C2.x); St.put(15, C1.y, C2.y, C1.z, C2.z);
    hw_barrier();      // the contact terms are in LDS
#if LM_H3_XBLOCKS
    helper_xblocks<0, 1>(St, XB_OUT);
    hw_barrier();      // B3: the cross blocks are in LDS
#endif
  }
}
#endif
#endif

// One physics sub-step of one env (4 lanes).  MODE 0: F is the robot base.  MODE 1: F is the plate, the
// robot base is fixed at (Rb, pb).
// CF 1 (the contact-force reporting kernels): cf[0..2] += the world-frame contact impulse on this lane's foot, cf[3] += 1 when
// the foot is loaded (lam_n > 0), both from the impulses of the sub-step's last pass.
// HW 1 (wavefront 0 of k_step_h2; locomotion, no DR, first pass on registers): the limb's bias terms come from the helper wavefront (helper_wave).
template <int MODE, int VAR, int DR, int CF = 0, int REG0 = 1, int HW = 0>
LM_DEV void substep(const lm_params* __restrict__ P, const float* th, const float* tl, int limb, const Stash& St,
                    FreeBody& F, const M3& Rfix, V3 pfix, float q[3], float qd[3], const float tgt[3], float tau_acc[3], const DrPhys& X, float* cf = nullptr) {
  const float dt = P->dt, kd = DR ? X.kd : P->kd;      // DR: this env's velocity gain (the block's kd unless the kd channel drew)
  const float cjv[3] = {VAR ? (DR ? X.cj[0] : P->joint_damping) : 0.f, VAR ? (DR ? X.cj[1] : P->joint_damping) : 0.f, VAR ? (DR ? X.cj[2] : P->joint_damping) : 0.f};
  const float tmax[3] = {DR ? X.tmax[0] : P->tau_max, DR ? X.tmax[1] : P->tau_max, DR ? X.tmax[2] : P->tau_max};
  const float mu_dr = DR ? X.mu : 0.f;      // the DrPhys X is shadowed by the contact rows inside the pass loop
  const bool mp_on = DR && MODE == 1 && X.mp_on;      // a plate mass channel is on (wave-uniform): per-env plate inertia instead of plate_si / plate_phi
  const float m_plate = mp_on ? X.m_plate : 0.f, s_plate = mp_on ? X.s_plate : 0.f;
  M3 Rf = quat_to_mat(F.q.w, F.q.x, F.q.y, F.q.z);
#ifdef LM_HELPER_WAVE
  static_assert(!HW || (MODE == 0 && !DR && LM_PASS0_REG && REG0), "the helper wavefront serves the un-randomised locomotion sub-step with its first pass on registers");
  if (HW) {      // what the helper needs of this sub-step's state; it starts behind the barrier
    St.put(HAND_IN, q[0], q[1], q[2], qd[0]); St.put(HAND_IN + 1, qd[1], qd[2], F.u.w.x, F.u.w.y); St.put(HAND_IN + 2, F.u.w.z, F.u.v.x, F.u.v.y, F.u.v.z);
    St.put(HAND_IN + 3, Rf.c0.z, Rf.c1.z, Rf.c2.z, HW == 2 ? F.p.z : 0.f);      // (HW 2: the base height, for the terms helper's gap)
    hw_barrier();
  }
#endif
  constexpr bool REG0_ = LM_PASS0_REG ? REG0 != 0 : false;     // first pass on registers (else: both passes read the stash back, the form before round 5)
  // read with the sub-step's other parameters, not inside the divergent phi < 0 branch (a cache round trip on every wavefront with a penetrating
  // foot).  Not in the kernels that keep the stash form: two more live registers cost k_step_w2 20 B of scratch
  const float baumgarte = REG0_ ? P->baumgarte : 0.f, max_depen_vel = REG0_ ? P->max_depen_vel : 0.f;
  float bn; PassTerms I;
  {
    M3 Rb; V3 pb; SV v0;
    if (MODE == 0) { Rb = Rf; pb = F.p; v0 = F.u; } else { Rb = Rfix; pb = pfix; v0 = sv(v3(0, 0, 0), v3(0, 0, 0)); }
    SV avp0 = sv(v3(0, 0, 0), DR ? mulT(Rb, -X.g) : P->gravity * row2(Rb));      // fictitious acceleration = -gravity
    LimbKin K; limb_kinematics(tl, q, qd, K);
    LimbDyn D;
    if (DR && X.mb_on) limb_dynamics<1>(tl, K, qd, v0, avp0, D, X.m_s, X.m_41, X.m_32);      // body-mass channel on (wave-uniform): per-env masses
    else if (HW) limb_dynamics<0, 1>(tl, K, qd, v0, avp0, D);      // the inertia chain; fcs and hq: the helper wavefront's, fetched by the pass
    else limb_dynamics(tl, K, qd, v0, avp0, D);
    LM_STAMP(1);
    if (MODE == 0) {
      // the hub body itself rides on limb 0's contribution to the quad reductions
      const float m0 = (limb == 0) ? 1.f : 0.f;
      SI I0 = hub_inertia(th);
      if (DR && X.mb_on) {
        // per-env hub mass m': the COM c = h / m and the inertia about it stay, so I_O' = I_O + (m' - m) (|c|^2 1 - c c^T) and h' = h m' / m.
        // In this form m' = m gives the table's values back bit for bit
        const V3 c = (1.0f / I0.m) * I0.h; const float dm = X.m_hub - I0.m, cc = dot(c, c);
        I0.xx = fmaf(dm, cc - c.x * c.x, I0.xx); I0.yy = fmaf(dm, cc - c.y * c.y, I0.yy); I0.zz = fmaf(dm, cc - c.z * c.z, I0.zz);
        I0.xy = fmaf(dm, -(c.x * c.y), I0.xy); I0.xz = fmaf(dm, -(c.x * c.z), I0.xz); I0.yz = fmaf(dm, -(c.y * c.z), I0.yz);
        I0.h = (X.m_hub / I0.m) * I0.h; I0.m = X.m_hub;
      }
      const V3 com0 = (1.0f / I0.m) * I0.h;
      I0.m *= m0; I0.h = m0 * I0.h; I0.xx *= m0; I0.yy *= m0; I0.zz *= m0; I0.xy *= m0; I0.xz *= m0; I0.yz *= m0;
      D.Isc = D.Isc + I0;
      if (!HW) D.fcs = D.fcs + I0 * avp0 + fcross(v0, I0 * v0);      // (HW: the helper wavefront adds the hub's bias term)
      if (DR) { V3 fh = m0 * mulT(Rb, X.f); D.fcs = D.fcs - sv(cross(com0, fh), fh); }      // randomised force on the base link, at its COM
    }
#ifdef LM_HELPER_WAVE
    if (HW == 2) {
      // k_step_h3: the inertia chain's terms only.  The contact geometry, the Jq dots and the hub rows are the terms helper's
      // (helper_wave_terms): the first pass reads them from stash slots 7-15 behind its barrier, and so does a second pass
      I.Fq0 = s6(D.Fq0); I.Fq1 = s6(D.Fq1); I.Fq2 = s6(D.Fq2);
      I.Ha[0] = D.H[0]; I.Ha[1] = D.H[1]; I.Ha[2] = D.H[2]; I.Ha[3] = D.H[3]; I.Ha[4] = D.H[4]; I.Ha[5] = D.H[5];
      I.hq[0] = I.hq[1] = I.hq[2] = 0.f; I.Jq0[0] = I.Jq0[1] = I.Jq0[2] = 0.f; I.j12[0] = I.j12[1] = I.j12[2] = sp2(0.f);
#pragma unroll
      for (int i = 0; i < 6; i++) { I.PB[i].p = sp2(0.f); I.PB[i].q = sp2(0.f); }
      I.Isc = D.Isc;
      pin_chain(I);
      stash_chain(St, I);
      bn = 0.f;
    }
#endif
    if (HW != 2) {
    // ---- contact geometry of this limb's tip
    V3 C0, C1, C2;        // contact axes (n, t1, t2) in hub coordinates
    float phi;
    if (MODE == 0) {
      // contact axes in hub coordinates: n = world z; t1 = the base's x axis projected onto the ground plane, t2 = n x t1.  The friction
      // basis turns with the robot, so the dynamics do not depend on its heading (exactly, even with the unconverged solver)
      C0 = row2(Rb);
      C1 = rsqrtf(fmaxf(1.0f - C0.x * C0.x, 1.0e-12f)) * v3(1.0f - C0.x * C0.x, -C0.x * C0.y, -C0.x * C0.z);
      C2 = cross(C0, C1);
      phi = pb.z + dot(C0, D.x) - P->tip_radius;
      D.x = fma3(-P->tip_radius, C0, D.x);      // from here on: the contact point on the sphere's surface (Jacobians are taken there)
    } else {
      V3 xw = pb + mul(Rb, D.x);
      V3 yc = mulT(Rf, xw - F.p);                // sphere centre, plate coordinates
      V3 y = yc - v3(P->plate_center[0], P->plate_center[1], P->plate_center[2]);
      // contact face = the slab face on the robot's side of the plate (robust to deep initial overlap)
      float sg = (mulT(Rf, pb - F.p).z - P->plate_center[2] >= 0.f) ? 1.f : -1.f;
      phi = sg * y.z - P->plate_half[2] - P->tip_radius;
      if (fabsf(y.x) > P->plate_half[0] || fabsf(y.y) > P->plate_half[1]) phi = 1.0e3f;
      // contact axes in plate coords: n=(0,0,sg) t1=(1,0,0) t2=(0,sg,0); in hub coords: Rb^T Rf axis
      M3 Mrp = mulTA(Rb, Rf);
      C0 = sg * Mrp.c2; C1 = Mrp.c0; C2 = sg * Mrp.c1;
      D.x = fma3(-P->tip_radius, C0, D.x);      // the contact point on the sphere's surface, hub coordinates ...
      V3 y0 = v3(yc.x, yc.y, yc.z - sg * P->tip_radius);      // ... and plate coordinates
      V3 a0 = v3(0, 0, sg), a1 = v3(1, 0, 0), a2 = v3(0, sg, 0);
      SV Tp0 = sv(-cross(y0, a0), -a0), Tp1 = sv(-cross(y0, a1), -a1), Tp2 = sv(-cross(y0, a2), -a2);
      // plate free motion
      SV up_free;
      if (mp_on) {      // per-env plate mass / inertia factor
        const V3 c = v3(P->plate_com[0], P->plate_com[1], P->plate_com[2]);
        const SI Ip = plate_inertia_env(P, m_plate, s_plate);
        SV hp = fcross(F.u, Ip * F.u);
        const V3 fg = m_plate * mulT(Rf, X.g);
        hp = hp - sv(cross(c, fg), fg);
        const PlateInvT<float> Q = plate_inv(P, m_plate, s_plate);
        V3 al, ac; plate_inv_apply<float>(Q, hp.w, hp.v, al, ac);
        up_free = F.u - dt * sv(al, ac);
      } else {
        SI Ip = load_si(P->plate_si);
        SV hp = fcross(F.u, Ip * F.u);
        V3 fg = DR ? P->plate_mass * mulT(Rf, X.g) : (-P->plate_mass * P->gravity) * row2(Rf);
        V3 c = v3(P->plate_com[0], P->plate_com[1], P->plate_com[2]);
        hp = hp - sv(cross(c, fg), fg);
        float Ph[6][6];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
          for (int j = 0; j < 6; j++) Ph[i][j] = P->plate_phi[6 * i + j];
        up_free = F.u - dt * mul66(Ph, hp);
      }
      // pass-invariant contact rows in the four-vector layout: PB[i].p = (up_free[i] | Tp0[i]), PB[i].q = (Tp1[i] | Tp2[i])
      if (!REG0_) {
        St.put(10, up_free.w.x, Tp0.w.x, up_free.w.y, Tp0.w.y); St.put(11, up_free.w.z, Tp0.w.z, up_free.v.x, Tp0.v.x); St.put(12, up_free.v.y, Tp0.v.y, up_free.v.z, Tp0.v.z);
        St.put(13, Tp1.w.x, Tp2.w.x, Tp1.w.y, Tp2.w.y); St.put(14, Tp1.w.z, Tp2.w.z, Tp1.v.x, Tp2.v.x); St.put(15, Tp1.v.y, Tp2.v.y, Tp1.v.z, Tp2.v.z);
      } else LM_PASS_ROWS(I, up_free, Tp0, Tp1, Tp2)
    }
    bn = (phi >= 0.f) ? phi / dt : REG0_ ? fmaxf(baumgarte * phi / dt, -max_depen_vel) : fmaxf(P->baumgarte * phi / dt, -P->max_depen_vel);
    // tip linear velocity per unit generalized rate, contact coordinates
    V3 e0 = K.s1.v + cross(K.s1.w, D.x);
    V3 e1 = D.j31.v + cross(D.j31.w, D.x);
    V3 e2 = D.j32.v + cross(D.j32.w, D.x);
    if (!REG0_) {
      // written straight from where they were computed: these kernels' register allocation is the one they had
#ifdef LM_WAVES2
      stash_sv3(St, 0, D.Fq0, D.Fq1, D.Fq2, D.Isc.xz, D.Isc.yz);
#else
      stash_sv3(St, 0, D.Fq0, D.Fq1, D.Fq2);
#endif
      St.put(5, D.H[0], D.H[1], D.H[2], D.H[3]); St.put(6, D.H[4], D.H[5], D.hq[0], D.hq[1]);
      St.put(7, D.hq[2], dot(C0, e0), dot(C0, e1), dot(C0, e2));
      St.put(8, dot(C1, e0), dot(C2, e0), dot(C1, e1), dot(C2, e1)); St.put(9, dot(C1, e2), dot(C2, e2), 0.f, 0.f);
      if (MODE == 0) {
        const V3 n0 = cross(D.x, C0), n1 = cross(D.x, C1), n2 = cross(D.x, C2);
        St.put(10, D.fcs.w.x, n0.x, D.fcs.w.y, n0.y); St.put(11, D.fcs.w.z, n0.z, D.fcs.v.x, C0.x); St.put(12, D.fcs.v.y, C0.y, D.fcs.v.z, C0.z);
        St.put(13, n1.x, n2.x, n1.y, n2.y); St.put(14, n1.z, n2.z, C1.x, C2.x); St.put(15, C1.y, C2.y, C1.z, C2.z);
        St.put(16, D.Isc.m, D.Isc.h.x, D.Isc.h.y, D.Isc.h.z); St.put(17, D.Isc.xx, D.Isc.yy, D.Isc.zz, D.Isc.xy);
#ifndef LM_WAVES2
        St.put(18, D.Isc.xz, D.Isc.yz, 0.f, 0.f);
#endif
      }
    } else {
#ifdef LM_HELPER_WAVE
      if (HW) {      // the helper wavefront's terms: not in I (the first pass fetches them where it needs them, the second pass below)
        D.fcs = sv(v3(0, 0, 0), v3(0, 0, 0)); D.hq[0] = D.hq[1] = D.hq[2] = 0.f;
      }
#endif
      I.Fq0 = s6(D.Fq0); I.Fq1 = s6(D.Fq1); I.Fq2 = s6(D.Fq2);
      I.Ha[0] = D.H[0]; I.Ha[1] = D.H[1]; I.Ha[2] = D.H[2]; I.Ha[3] = D.H[3]; I.Ha[4] = D.H[4]; I.Ha[5] = D.H[5];
      I.hq[0] = D.hq[0]; I.hq[1] = D.hq[1]; I.hq[2] = D.hq[2];
      // Jq = contact-coordinate tip velocity per unit joint rate: row 0 plain, rows 1 and 2 interleaved (Jq[1][c] | Jq[2][c])
      I.Jq0[0] = dot(C0, e0); I.Jq0[1] = dot(C0, e1); I.Jq0[2] = dot(C0, e2);
      I.j12[0] = mk2(dot(C1, e0), dot(C2, e0)); I.j12[1] = mk2(dot(C1, e1), dot(C2, e1)); I.j12[2] = mk2(dot(C1, e2), dot(C2, e2));
      if (MODE == 0) {
        // hub rows Jb_r = [x x C_r ; C_r] of the three contact axes and the limb's bias wrench, in the four-vector layout:
        // PB[i].p = (fcs[i] | Jb0[i]), PB[i].q = (Jb1[i] | Jb2[i]); and the limb's composite inertia
        const SV Jb0 = sv(cross(D.x, C0), C0), Jb1 = sv(cross(D.x, C1), C1), Jb2 = sv(cross(D.x, C2), C2);
        LM_PASS_ROWS(I, D.fcs, Jb0, Jb1, Jb2)
        I.Isc = D.Isc;
      }
      pin_terms<MODE>(I);
      stash_terms<MODE>(St, I);
    }
    }
  }

  LM_STAMP(2);
  // effort mode (RobotOmni.take_action, robot.py:455-459): tgt IS the joint torque, gains off = the constant-torque branch from the start
  const bool effort = (VAR == 0) && P->drive_mode == LM_DRIVE_EFFORT;
  bool sat[3] = {effort, effort, effort}; float tsat[3] = {effort ? tgt[0] : 0.f, effort ? tgt[1] : 0.f, effort ? tgt[2] : 0.f};
  // PD-actuator families: the reference evaluates  clamp(kp (q* - q) - kd qd, +-max_effort)  on the state BEFORE the sub-step and holds it
  // (quadruped_pose_control_custom_controller.py:289-293), so which joints sit on the limit is known up front: those get the constant limit
  // torque, the others the implicit form of the same PD law, in ONE pass.  The implicit (end-of-step) torque of an unsaturated joint leaves the
  // limit in 0.02 % of the joint-sub-steps under random actions; lm_params.pd_second_pass = 1 puts those on the limit too and solves again.  That
  // happens in 1-3 % of the wavefront-sub-steps (tools/pass2_count.py), but a step lasts as long as its slowest wavefront and one of the 256
  // nearly always has one: +6 us per step, which is why it is off by default.
  // (Variant 0 with a finite tau_max limits the force of an implicit drive, which only the solve can tell: two passes.)
  if (VAR) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float tau = kd * (tgt[a] - qd[a]);
      const bool hi_ = tau > tmax[a], lo_ = tau < -tmax[a];
      sat[a] = hi_ || lo_; tsat[a] = hi_ ? tmax[a] : -tmax[a];
    }
  }
  float qdn[3]; SV un; float lamc[3] = {0.f, 0.f, 0.f};
  // whether a second pass is due after the first (wave-uniform): some joint of some env newly sits on its limit
  auto second_pass_due = [&]() -> bool {
    if (effort || (VAR != 0 && !P->pd_second_pass)) return false;
    int any = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float tau = kd * (tgt[a] - qdn[a]);
      const bool hi_ = tau > tmax[a], lo_ = tau < -tmax[a];
      if (VAR) {                             // joints already on the limit (the pre-step decision) stay there
        const bool nw = !sat[a] && (hi_ || lo_);
        tsat[a] = nw ? (hi_ ? tmax[a] : -tmax[a]) : tsat[a]; sat[a] = sat[a] || nw; any |= nw ? 1 : 0;
      } else {
        sat[a] = hi_ || lo_; tsat[a] = hi_ ? tmax[a] : -tmax[a]; any |= (hi_ || lo_) ? 1 : 0;
      }
    }
    any = quad_sum_i(any);
#ifdef LM_COUNT_PASS2
    { const bool wa = __any(any); if ((threadIdx.x & 63) == 0) { atomicAdd(&lm_dbg_pass2[0], 1u); if (wa) atomicAdd(&lm_dbg_pass2[1], 1u); } }
#endif
    return __any(any);                       // wave-uniform: false when nobody saturated
  };
  if (!REG0_) {
    // both passes from the stash (the form before round 5)
    for (int pass = 0; pass < 2; pass++) {
      unstash_terms<MODE>(St, I);
      substep_pass<MODE, VAR, DR, CF>(P, limb, F, I, dt, kd, cjv, sat, tsat, tgt, qd, bn, mu_dr, mp_on, m_plate, s_plate, qdn, un, lamc);
      if (pass == 0 && !second_pass_due()) break;
    }
  } else {
    // first pass: on the registers just computed.  Second pass: reloaded from the stash, under a wave-uniform branch; envs without saturation
    // redo the identical unsaturated solve in it (same result)
    substep_pass<MODE, VAR, DR, CF, HW>(P, limb, F, I, dt, kd, cjv, sat, tsat, tgt, qd, bn, mu_dr, mp_on, m_plate, s_plate, qdn, un, lamc, &St);
    if (second_pass_due()) {
      unstash_terms<MODE>(St, I);
#ifdef LM_HELPER_WAVE
      if (HW) {      // the helper's terms are still in its slots: it writes them again behind the next sub-step's first barrier
        const float4 b0 = St.get(HAND_OUT), b1 = St.get(HAND_OUT + 1), b2 = St.get(HAND_OUT + 2);
        I.PB[0].p.x = b0.x; I.PB[1].p.x = b0.y; I.PB[2].p.x = b0.z; I.PB[3].p.x = b0.w; I.PB[4].p.x = b1.x; I.PB[5].p.x = b1.y;
        I.hq[0] = b1.z; I.hq[1] = b1.w; I.hq[2] = b2.x;
        if (HW == 2) bn = St.get(9).z;      // the terms helper's approach rate rides in the spare half of slot 9
      }
#endif
      substep_pass<MODE, VAR, DR, CF>(P, limb, F, I, dt, kd, cjv, sat, tsat, tgt, qd, bn, mu_dr, mp_on, m_plate, s_plate, qdn, un, lamc);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {      // driven joints are speed-limited like PhysX's maxJointVelocity (config_module_joints.py:11,61-69)
    // the LOGGED drive torque (observation 88, mechanical power): clipped like the reference's (…custom_controller.py:289-293); the implicit torque
    // applied to an unsaturated joint can exceed the limit in 0.02 % of the joint-sub-steps when pd_second_pass = 0 - dynamics only, never logged
    if (VAR) tau_acc[a] += sat[a] ? tsat[a] : fminf(fmaxf(kd * (tgt[a] - qdn[a]), -tmax[a]), tmax[a]);
    const float vm = DR ? X.vmax[a] : P->max_joint_vel;
    float v = fminf(fmaxf(qdn[a], -vm), vm);
    qd[a] = v; q[a] = fmaf(dt, v, q[a]);
  }
  if (CF) {
    // the contact axes again, in the world frame (R_b C_r of the hub-coordinate axes above), from Rf / sg of the state before the sub-step: nine
    // registers less across the pass loop than keeping C0, C1, C2.  Locomotion: R_b C0 = z exactly, R_b C1 = the base's x axis without its z part
    // Every product-sum below is an explicit fmaf: an expression like a b - c d can be contracted two ways, and the records of k_step_cf and
    // k_substeps_cf must agree bit for bit whatever the compiler would choose in either
    if (MODE == 0) {
      const float s = rsqrtf(fmaxf(fmaf(-Rf.c0.z, Rf.c0.z, 1.0f), 1.0e-12f));
      cf[0] = fmaf(s, fmaf(lamc[1], Rf.c0.x, -(lamc[2] * Rf.c0.y)), cf[0]);
      cf[1] = fmaf(s, fmaf(lamc[1], Rf.c0.y, lamc[2] * Rf.c0.x), cf[1]);
      cf[2] += lamc[0];
    } else {
      const float sg = (mulT(Rf, pfix - F.p).z - P->plate_center[2] >= 0.f) ? 1.f : -1.f;      // n = sg x plate z, t1 = plate x, t2 = n x t1 = sg x plate y
      const float ln = sg * lamc[0], l2 = sg * lamc[2];
      cf[0] += fmaf(ln, Rf.c2.x, fmaf(lamc[1], Rf.c0.x, l2 * Rf.c1.x));
      cf[1] += fmaf(ln, Rf.c2.y, fmaf(lamc[1], Rf.c0.y, l2 * Rf.c1.y));
      cf[2] += fmaf(ln, Rf.c2.z, fmaf(lamc[1], Rf.c0.z, l2 * Rf.c1.z));
    }
    cf[3] += lamc[0] > 0.f ? 1.f : 0.f;
  }
  F.u = un;
  integrate_free(F, Rf, dt);
  LM_STAMP(5);
}

// the contact record of a launch (LM_PTR_CONTACT, float [LM_CONTACT_ROWS][N]): the mean force on this lane's foot over the n sub-steps it ran and
// the share of them with the foot loaded.  Lanes of one limb write 16 consecutive envs of a row: four stores per lane, 16 row segments per wavefront
LM_DEV void store_contact(float* rec, int N, int env, int limb, bool active, const float cf[4], int n, float dt) {
  if (!active || n <= 0) return;
  const float sc = 1.0f / ((float)n * dt);
  rec[(size_t)(3 * limb + 0) * N + env] = cf[0] * sc; rec[(size_t)(3 * limb + 1) * N + env] = cf[1] * sc; rec[(size_t)(3 * limb + 2) * N + env] = cf[2] * sc;
  rec[(size_t)(12 + limb) * N + env] = (float)((double)cf[3] / (double)n);      // exactly rounded k / n (the build's fp32 division is the 1-ulp reciprocal)
}
