// Third translation unit of liblm_engine.so: the step with a helper wavefront (k_step_h2) and its launcher.  Up to 8192 envs on MI355X the
// one-wavefront workgroups of k_step leave at least half of the SIMDs without a wavefront, and the kernel is bound by the single wavefront's
// own instruction stream.  k_step_h2 runs workgroups of two wavefronts: wavefront 0 is k_step's step_body, wavefront 1 computes the limb bias
// terms of every locomotion sub-step beside it on another SIMD (helper_wave, lm_dynamics.h).  LM_HELPER_WAVE gives the step's
// device headers the seven hand-off slots behind the stash.  A separate unit so that the kernels of lm_engine.hip keep their register
// allocation and code layout; lm_step dispatches it while two wavefronts per workgroup still find a SIMD each (lm_create: h2_max_envs).
#ifndef LM_HELPER_WAVE
#define LM_HELPER_WAVE 1
#endif
#undef LM_STAMPS              // diagnostic switches of the whole-library builds do not apply to this unit (their device globals live in lm_engine.hip)
#undef LM_COUNT_PASS2
#undef LM_WAVES2
#undef LM_PASS0_STASH
#include "lm_step.h"

// un-randomised velocity-drive kinds 0 and 1, no contact reporting (the engines k_step serves)
__global__ void __launch_bounds__(128) k_step_h2(StepArgs A) {
  LM_STEP_SMEM(64)
  if (threadIdx.x >= 64) {
    // the helper returns at once where no sub-step needs it: a manipulation block, no sub-steps, no env.  All three are wave-uniform and read
    // from what wavefront 0 reads them from
    const int nsub = (A.nsub < 0) ? P->substeps : A.nsub;
    if (kind != 0 || env0 >= A.N) return;
    helper_wave(P, sTab, sStash, threadIdx.x - 64, nsub);
    return;
  }
  if (kind == 0) step_body<0, 0, 0, 0, 0, 1, 1>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 0, 0>(A, P, sTab, sObs, sSt, sStash);
}
extern "C" __attribute__((visibility("hidden"))) void lm_internal_launch_step_h2(const StepArgs* A, int nblocks, hipStream_t s) {
  hipLaunchKernelGGL(k_step_h2, dim3(nblocks), dim3(128), 0, s, *A);
}
