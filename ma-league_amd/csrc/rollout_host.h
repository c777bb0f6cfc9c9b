// rollout_host.h -- host-side argument checks and launch helpers shared by the rollout entry points
// (rollout.hip, rollout_policy.hip, crossplay.hip); file-local in each, like rollout_env_device.h.
#pragma once
#include "../../include/maleague.h"
#include "mlg_host.h"

namespace {

constexpr int LDS_LIMIT_BYTES = 160 * 1024;

int check_spec(const MlgEnvSpec* s) {
    MLG_REQUIRE(s != nullptr, "null spec");
    MLG_REQUIRE(s->U >= 2 && s->U <= MLG_MAXU, "spec.U=%d out of range [2, %d]", s->U, MLG_MAXU);
    MLG_REQUIRE(s->n_agents >= 1 && s->n_agents <= s->U, "spec.n_agents=%d invalid", s->n_agents);
    MLG_REQUIRE(s->n_actions == MLG_ACT_BASE + s->U, "spec.n_actions must be 5+U");
    MLG_REQUIRE(s->grid >= 2 && s->grid <= 4096, "spec.grid=%d invalid", s->grid);
    MLG_REQUIRE(s->episode_limit >= 1 && s->episode_limit < 65535, "spec.episode_limit invalid");
    MLG_REQUIRE(s->policy_team == 0 || s->policy_team == 1, "spec.policy_team invalid");
    for (int u = 0; u < s->U; ++u) {
        MLG_REQUIRE(s->team[u] == 0 || s->team[u] == 1, "unit %d team invalid", u);
        MLG_REQUIRE(s->role[u] >= 0 && s->role[u] <= 2, "unit %d role invalid", u);
        MLG_REQUIRE(s->melee[u] == 0 || s->melee[u] == 1, "unit %d attack type invalid", u);
    }
    for (int a = 0; a < s->n_agents; ++a)
        MLG_REQUIRE(s->agent_unit[a] >= 0 && s->agent_unit[a] < s->U, "agent %d unit invalid", a);
    return 0;
}

int check_state(const MlgEnvState* st) {
    MLG_REQUIRE(st && st->x && st->y && st->hp && st->t && st->episode, "env state has null pointers");
    MLG_REQUIRE(st->B >= 1, "env state B=%d", st->B);
    return 0;
}

int check_rollout_batch(const MlgBatch* batch, const MlgEnvSpec* spec, const MlgEnvState* st, const char* who) {
    MLG_REQUIRE(batch, "%s: null batch", who);
    MLG_REQUIRE(batch->state && batch->obs && batch->actions && batch->avail && batch->reward && batch->terminated &&
                    batch->actions_onehot && batch->filled,
                "%s: batch has null tensors", who);
    MLG_REQUIRE(batch->B == st->B, "%s: batch B=%d != env B=%d", who, batch->B, st->B);
    MLG_REQUIRE(batch->rows == nullptr, "%s: sampled (rows) views are read-only; use ring mode to write slots", who);
    MLG_REQUIRE(batch->T1 == spec->episode_limit + 1, "%s: batch T1=%d != episode_limit+1=%d", who, batch->T1,
                spec->episode_limit + 1);
    MLG_REQUIRE(batch->ring_size == 0 || (batch->ring_size >= batch->B && batch->ring_slot0 >= 0 &&
                                          batch->ring_slot0 < batch->ring_size),
                "%s: bad ring (slot0=%d size=%d B=%d)", who, batch->ring_slot0, batch->ring_size, batch->B);
    return 0;
}

// Raises the kernel's dynamic LDS limit when the launch needs more than the 64 KiB default.
template <typename K>
int allow_lds(K kern, size_t bytes, const char* who) {
    if (bytes <= 64 * 1024) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)bytes);
    if (e != hipSuccess) return mlg::fail("%s: LDS attribute (%zu B): %s", who, bytes, hipGetErrorString(e));
    return 0;
}

}  // namespace
