// osc_kin_model.hpp -- the kinematics model handle (include/osc_kinematics.h, osc_kin_model):
// the descriptor it was created from, the derived tables on the host and their device copy.
// Created / destroyed by osc_kinematics.hip; read by the units that launch on its tables
// (osc_kinematics.hip, osc_rollout.hip).
#pragma once
#include "osc_batch.h"
#include "osc_kin_device.hpp"
#include "osc_kinematics.h"

struct osc_kin_model {
  osc_kin_desc desc;
  osc_kin::KinDev host;
  osc_kin::KinDev* dev;
  int device;
};

namespace osc_kin {

// The workspace of a joint-state tick (osc_qpos_workspace_bytes): [M | C | J | b | reduced-QP
// workspace], each section 256-B aligned (byte offsets).
struct QposWorkspace {
  size_t m, c, j, b, ws, ws_bytes, total;
  static size_t align256(size_t n) { return (n + 255) & ~static_cast<size_t>(255); }
  QposWorkspace(const osc_model* model, const KinDev& k, int32_t nenv) {
    const size_t n = static_cast<size_t>(nenv);
    m = 0;
    c = m + align256(sizeof(double) * n * k.nv * k.nv);
    j = c + align256(sizeof(double) * n * k.nv);
    b = j + align256(sizeof(double) * n * 6 * k.nsite * k.nv);
    ws = b + align256(sizeof(double) * n * 6 * k.nsite);
    ws_bytes = 0;
    osc_workspace_bytes(model, nenv, &ws_bytes);
    total = ws + align256(ws_bytes);
  }
};

}  // namespace osc_kin
