// osc_kin_model.hpp -- the kinematics model handle (include/osc_kinematics.h, osc_kin_model):
// the descriptor it was created from, the derived tables on the host and their device copy.
// Created / destroyed by osc_kinematics.hip; read by the units that launch on its tables
// (osc_kinematics.hip, osc_rollout.hip).
#pragma once
#include "osc_kin_device.hpp"
#include "osc_kinematics.h"

struct osc_kin_model {
  osc_kin_desc desc;
  osc_kin::KinDev host;
  osc_kin::KinDev* dev;
  int device;
};
