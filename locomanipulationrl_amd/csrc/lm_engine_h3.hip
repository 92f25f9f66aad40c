// Fourth translation unit of liblm_engine.so: the step with two helper wavefronts (k_step_h3) and its launcher.  Up to 16 x CUs envs (4096 on
// MI355X: one workgroup per CU; with 466 registers a wavefront has a SIMD to itself) a third SIMD of every CU is idle.  k_step_h3 runs workgroups of three wavefronts: wavefront 0 is k_step's
// step_body, wavefront 1 is k_step_h2's helper_wave (the limb bias terms), wavefront 2 computes the contact geometry, the Jq dots and the hub
// rows of every locomotion sub-step (helper_wave_terms, lm_dynamics.h), which wavefront 0 - bound by its own instruction
// stream - then no longer issues, and streams the staged obs / states of a full wavefront out at the end of the step (helper_write_outputs,
// lm_task.h; -DLM_H3_OUT_HELPER=0 builds the kernel without that, for A/B).  LM_HELPER_WAVE 2 gives the step's device headers the hand-off slots and the terms helper.  A separate unit
// so that the kernels of the other units keep their register allocation and code layout; lm_step dispatches it up to h3_max_envs (lm_create).
//
// -DLM_H3_TAIL_STATE (1 by default; 0 builds the kernel without it and without its barrier, for A/B): wavefront 1, done with its last sub-step while
// wavefront 0 still factors and sweeps, fetches the task-layer state (19 words per lane; in a resetting wavefront the goal draw and the reset
// values) into five stash slots of its own and ends behind one more barrier, R1, behind which wavefront 0 reads them (helper_task_state, lm_step.h).
// Barriers of the tail, per wavefront: 0: R1 - output barrier; 1: R1, ends; 2: R1 - output barrier.
//
// -DLM_H3_XBLOCKS (1 by default; 0 builds the kernel without it and without its barrier, for A/B): behind the second barrier of every sub-step the
// two helpers, which would otherwise wait for the next sub-step, run the pass's elimination and hub solve on the three contact columns and two
// of the four raw cross blocks of the contact operator each, from K and the hub factor that wavefront 0 publishes in front of that barrier, and
// hand the blocks back behind a third barrier of the sub-step, B3 (helper_xblocks, lm_dynamics.h).  Barriers of a sub-step, in all three
// wavefronts: first - second - B3; a second pass has none.
#ifndef LM_HELPER_WAVE
#define LM_HELPER_WAVE 2
#endif
#ifndef LM_H3_XBLOCKS
#define LM_H3_XBLOCKS 1
#endif
#ifndef LM_H3_OUT_HELPER
#define LM_H3_OUT_HELPER 1
#endif
#ifndef LM_H3_TAIL_STATE
#define LM_H3_TAIL_STATE 1
#endif
#undef LM_STAMPS            // diagnostic switches of the whole-library builds do not apply to this unit (their device globals live in lm_engine.hip)
#undef LM_COUNT_PASS2
#undef LM_WAVES2
#undef LM_PASS0_STASH
#include "lm_step.h"

// un-randomised velocity-drive kinds 0 and 1, no contact reporting (the engines k_step serves)
__global__ void __launch_bounds__(192) k_step_h3(StepArgs A) {
  LM_STEP_SMEM(64)
  if (threadIdx.x >= 64) {
    // the helpers return at once where no sub-step needs them: a manipulation block, no sub-steps, no env.  All three are wave-uniform and read
    // from what wavefront 0 reads them from
    const int nsub = (A.nsub < 0) ? P->substeps : A.nsub;
    if (kind != 0 || env0 >= A.N) return;
    if (threadIdx.x >= 128) {
      helper_wave_terms(P, sTab, sStash, threadIdx.x - 128, nsub);
      // behind the last sub-step (also with no sub-step at all) this wavefront passes R1 with the other two, then waits at one more barrier,
      // which wavefront 0 passes once the outputs are staged in LDS, and streams them out; wavefront 1 has ended by then and no longer counts
      if (LM_H3_TAIL_STATE) hw_barrier();      // R1
      if (LM_H3_OUT_HELPER) helper_write_outputs<64>(P, A.W, A.N, env0, threadIdx.x - 128, sObs, sSt);
    } else {
      helper_wave(P, sTab, sStash, threadIdx.x - 64, nsub);
      if (LM_H3_TAIL_STATE) helper_task_state(A, P, sStash, threadIdx.x - 64);
    }
    return;
  }
  if (kind == 0) step_body<0, 0, 0, 0, 0, 1, 2, LM_H3_OUT_HELPER, 0, LM_H3_TAIL_STATE>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 0, 0>(A, P, sTab, sObs, sSt, sStash);
}
extern "C" __attribute__((visibility("hidden"))) void lm_internal_launch_step_h3(const StepArgs* A, int nblocks, hipStream_t s) {
  hipLaunchKernelGGL(k_step_h3, dim3(nblocks), dim3(192), 0, s, *A);
}
