// coma_device.h -- what the COMA kernels share (coma.hip, rollout_policy.hip).
#pragma once
#include "mlg_device.h"

// Counter-RNG purpose of the multinomial policy draw. 1-3 are mlg_device.h's (spawn, epsilon coin,
// random action), 4 the entity env's team draw (refil_device.h).
enum { MLG_PURPOSE_POLICY = 5 };
