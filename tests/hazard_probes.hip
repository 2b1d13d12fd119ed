// One small kernel per producer -> consumer pair of tools/check_dpp_hazards.py RULES, in builtins
// and plain C++ only: the compiler pads these pairs in its own code, so its listing of this file
// says how many wait states each needs on the target (tests/test_hazard_rules.py counts them and
// compares with the table).  Each kernel leaves the compiler nothing else to put between the pair:
// the consumer depends on the producer alone, and whatever else the kernel needs comes before it.
// Never launched.
#include <hip/hip_runtime.h>

// VALU writes a VGPR -> DPP reads it as its shuffled source
extern "C" __global__ void probe_valu_dpp(int* o, int a) {
  const int x = a + threadIdx.x;
  o[threadIdx.x] = __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
}

// v_cmp writes VCC -> v_cndmask reads VCC
extern "C" __global__ void probe_vcc_mask(float* o, const float* p, float a, float b) {
  const float x = p[threadIdx.x];
  o[threadIdx.x] = x > a ? b : x;
}

// v_cmp writes VCC -> a VALU instruction reads it as a plain operand
extern "C" __global__ void probe_vcc_operand(unsigned* o, const float* p, float a) {
  const float x = p[threadIdx.x];
  const unsigned long long m = __builtin_amdgcn_ballot_w64(x > a);
  o[threadIdx.x] = static_cast<unsigned>(m) + threadIdx.x;
}

// v_cmp writes an SGPR pair -> v_cndmask reads it as its wave mask (VCC is held by m1, which is
// live across the pair, and the second compare depends on the first select)
extern "C" __global__ void probe_sgpr_mask(float* o, const float* p, float a, float b) {
  const float x = p[threadIdx.x], y = p[threadIdx.x + 64];
  const bool m1 = y > b;
  const float r = m1 ? x : y;
  const bool m0 = r > a;
  const float q = m0 ? r : x;
  o[threadIdx.x] = m1 ? q : y;
}

// v_readlane writes an SGPR -> a VALU instruction reads it
extern "C" __global__ void probe_lane_sgpr_operand(float* o, const float* p, float a) {
  const float x = p[threadIdx.x] * a;
  o[threadIdx.x] = __builtin_amdgcn_readlane(x, 5);
}

// a transcendental writes a VGPR -> a VALU instruction reads it
extern "C" __global__ void probe_trans_valu(double* o, const double* p) {
  const double x = p[threadIdx.x];
  o[threadIdx.x] = __builtin_amdgcn_rcp(x) * x;
}

// VALU writes a VGPR -> v_readfirstlane / v_readlane reads it (the producer is a DPP move: a
// plain add or multiply is moved behind the lane read)
extern "C" __global__ void probe_valu_readfirstlane(int* o, const int* p) {
  const int x = __builtin_amdgcn_update_dpp(0, p[threadIdx.x], 0x111, 0xf, 0xf, false);
  o[0] = __builtin_amdgcn_readfirstlane(x);
}
extern "C" __global__ void probe_valu_readlane(int* o, const int* p) {
  const int x = __builtin_amdgcn_update_dpp(0, p[threadIdx.x], 0x111, 0xf, 0xf, false);
  o[0] = __builtin_amdgcn_readlane(x, 5);
}

// v_readfirstlane writes an SGPR -> v_readlane takes it as its lane select
extern "C" __global__ void probe_sgpr_lane_select(int* o, const int* p) {
  const int x = p[threadIdx.x];
  const int s = __builtin_amdgcn_readfirstlane(x);
  o[0] = __builtin_amdgcn_readlane(x, s);
}

// a write of EXEC -> DPP / v_readlane: the divergent branch is how plain C++ changes EXEC.  On
// this target the compiler does it with scalar instructions, which none of the rules covers; the
// test requires that, so a toolchain that starts writing EXEC from the VALU has to be probed.
extern "C" __global__ void probe_exec_dpp(int* o, const int* p, int a) {
  const int x = p[threadIdx.x];
  if (x > a) o[threadIdx.x] = __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
}
extern "C" __global__ void probe_exec_readlane(int* o, const int* p, int a) {
  const int x = p[threadIdx.x];
  if (x > a) o[threadIdx.x] = __builtin_amdgcn_readlane(x, 3);
}
