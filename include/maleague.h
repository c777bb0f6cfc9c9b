/*
 * maleague.h -- C ABI of the MI355X-native hot path of PMatthaei/ma-league (libmaleague.so, gfx950).
 *
 * Every entry point takes plain device pointers (HBM, allocated by the caller: PyTorch's caching
 * allocator in the Python host package), sizes, and a hipStream_t passed as void*. Kernels are
 * enqueued on that stream; no call allocates, frees or synchronises (graph-capturable), except
 * where noted. Return value: 0 on success, nonzero on error; mlg_last_error() holds the message.
 *
 * Reference interfaces each entry point replaces (file:line in /root/reference):
 *   mlg_rollout        ParallelStepper.run / reset  src/steppers/parallel_stepper.py:82-216
 *   mlg_rollout_selfplay SelfPlayParallelStepper.run src/steppers/self_play_parallel_stepper.py:73-201
 *                      (+ SelfPlayStepper.run src/steppers/self_play_stepper.py:44-147,
 *                         build_pre_transition_data src/steppers/utils/stepper_utils.py:4-24)
 *                      + EnvWorker step/reset       src/steppers/utils/env_worker_process.py:27-71
 *                      + BasicMAC.select_actions    src/marl/controllers/basic_controller.py:29-36
 *                      + EpsilonGreedy.select       src/marl/components/action_selectors.py:44-62
 *                      + maenv TeamsEnv.step/get_obs/get_state/get_avail_actions (external)
 *   mlg_env_reset      EnvWorker "reset" command    src/steppers/utils/env_worker_process.py:54-60
 *   mlg_env_step       EnvWorker "step" command     src/steppers/utils/env_worker_process.py:32-53
 *   mlg_env_observe    TeamsEnv get_obs/get_state/get_avail_actions (env_worker_process.py:41-42)
 *   mlg_agent_forward  DRQNAgentNetwork.forward     src/marl/modules/agents/drqn_agent.py:29-35
 *   mlg_mac_forward    BasicMAC.forward + _build_inputs  src/marl/controllers/basic_controller.py:38-50,80-92
 *   mlg_select_actions EpsilonGreedyActionSelector.select src/marl/components/action_selectors.py:44-62
 *   mlg_pack_agent     (layout step feeding the above; no reference counterpart)
 *   mlg_ff_forward     DQNAgentNetwork.forward      src/marl/modules/agents/dqn_agent.py:34-37
 *   mlg_ff_mac_forward / mlg_rollout_ff  BasicMAC.forward / ParallelStepper.run with agent: dqn (Feed-forward agent
 *                      section below)
 *   mlg_qmix_forward   QMixer.forward               src/marl/modules/mixers/qmix.py:41-59
 *   mlg_agent_backward / mlg_qmix_backward  loss.backward() through the two above, one step / one call at a time
 *                      (src/marl/learners/q_learner.py:47-52,103 with any loss)
 *   mlg_crossplay_rollout  JointPolicyCorrelationEvaluationRun.evaluate_instances (all pairs in one launch)
 *                      src/runs/evaluation/jpc_eval_run.py:62-89
 *   mlg_rollout_selfplay_mix  mlg_rollout_selfplay with one away policy and roster per 16 envs (a league match against
 *                      an opponent mixture; no reference counterpart: its matches are single-env episodes)
 *   mlg_refil_*      REFIL (config 5): see the REFIL section below
 *   mlg_policy_probs   MultiAgentController._softmax src/marl/controllers/multi_agent_controller.py:78-99
 *   mlg_select_multinomial MultinomialActionSelector.select src/marl/components/action_selectors.py:11-32
 *   mlg_rollout_policy ParallelStepper.run with a pi_logits MAC (the two above inside mlg_rollout's run)
 *   mlg_coma_critic_train COMALearner._train_critic  src/marl/learners/coma_learner.py:10-21,121-169
 *                      + COMACritic                  src/marl/modules/critics/coma.py:22-73
 *   mlg_coma_target_update the target-critic update  src/marl/learners/coma_learner.py:104-106
 *   mlg_coma_policy_loss the COMA actor loss         src/marl/learners/coma_learner.py:75-96
 *   mlg_qlearner_*     QLearner.train               src/marl/learners/q_learner.py:34-131
 *                      + clip_grad_norm_ + RMSprop.step (q_learner.py:104-105, learner.py:25-31)
 *   mlg_per_*          Memory / BinarySumTree / PrioritizedReplayBuffer
 *                      src/marl/components/replay_buffers/prioritized_replay_buffer.py:8-224
 */
#ifndef MALEAGUE_H
#define MALEAGUE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLG_MAXU 64 /* max units per env (large.json has 50) */

/* Frozen synthetic TeamsEnv spec v1. Built on the host from env_args. */
typedef struct {
    int32_t U;             /* total units (both teams) */
    int32_t n_agents;      /* policy-controlled units = env_info["n_agents"] */
    int32_t n_actions;     /* 5 + U */
    int32_t grid;          /* env_args.grid_size */
    int32_t episode_limit; /* env_info["episode_limit"] */
    int32_t stochastic;    /* env_args.stochastic_spawns */
    int32_t policy_team;   /* first non-scripted plan team (stepper_utils.py:48-55) */
    int32_t n_policy_teams;
    int32_t team[MLG_MAXU];
    int32_t role[MLG_MAXU];  /* TANK 0, HEALER 1, ADC 2 */
    int32_t melee[MLG_MAXU]; /* RANGED 0, MELEE 1 */
    int32_t agent_unit[MLG_MAXU];
    int32_t scripted[2];
    uint64_t seed; /* per-env key = seed * 2^32 + env_index */
} MlgEnvSpec;

/* Device-resident env state, SoA, [B][U] int32 + per-env counters. */
typedef struct {
    int32_t *x, *y, *hp;   /* [B*U] */
    int32_t *t;            /* [B] step index within episode */
    uint32_t *episode;     /* [B] episodes started (RNG stream counter) */
    int32_t B;
} MlgEnvState;

/* EpisodeBatch transition tensors (scheme of ma_experiment.py:99-118), all [B][T1][...] row-major. */
typedef struct {
    float *state;          /* [B][T1][S] */
    float *obs;            /* [B][T1][N][d_obs] */
    int64_t *actions;      /* [B][T1][N][1] */
    int32_t *avail;        /* [B][T1][N][A] */
    float *reward;         /* [B][T1][1] */
    uint8_t *terminated;   /* [B][T1][1] */
    float *actions_onehot; /* [B][T1][N][A] */
    int64_t *filled;       /* [B][T1][1] */
    int32_t B, T1;
    /* Ring mode (mlg_rollout only): env b writes slot (ring_slot0 + b) % ring_size of tensors that hold
     * ring_size slots (the replay buffer itself -- zero-copy insert); full_write = 1 makes the kernel write
     * every byte of the slots it owns (zeros included), so the caller need not zero-initialise them. */
    int32_t ring_slot0, ring_size, full_write;
    /* Sampled view (learner entry points only): episode b lives in slot rows[b] of tensors holding more
     * slots (the replay buffer itself -- no gather copy); nullptr = identity. */
    const int32_t *rows;
    /* Full-write mode, optional [ring_size] (or [B] without a ring): per slot, the exclusive end of the rows
     * that may hold non-zero data (>= T1 = unknown, e.g. a fresh or externally written buffer). The rollout
     * zeroes only rows [L + 1, slot_extent) of a slot whose new episode has length L instead of [L + 1, T1),
     * and stores slot_extent = L + 1. nullptr = zero every tail row. */
    int32_t *slot_extent;
} MlgBatch;

/* Per-run episode summary written by mlg_rollout. */
typedef struct {
    int32_t *ep_len;   /* [B] env steps taken (t_env increment per env) */
    float *ret;        /* [B] episode return of the policy team (reward[0]) */
    int32_t *won;      /* [B][2] battle_won, policy team first */
    int32_t *draw;     /* [B] */
    uint64_t *agent_rows; /* optional [1], accumulated: agent rows the launch ran through the MFMA cell
                             (16-row tiles, padding included; living agents of running envs only) */
    float *ret_away;   /* optional [B] (mlg_rollout_selfplay): episode return of the away team (reward[1]) */
} MlgRunInfo;

/* Agent weights in canonical nn.Module layout (state_dict of DRQNAgentNetwork). */
typedef struct {
    const float *fc1_w, *fc1_b;     /* [H][d_in], [H] */
    const float *w_ih, *b_ih;       /* [3H][H], [3H] */
    const float *w_hh, *b_hh;       /* [3H][H], [3H] */
    const float *fc2_w, *fc2_b;     /* [A][H], [A] */
} MlgAgentParams;

typedef struct {
    int32_t d_obs, n_actions, n_agents, hidden, d_in;
    int32_t obs_last_action, obs_agent_id;
} MlgAgentDims;

/* Size in floats of the packed agent weight block used by the kernels. */
int64_t mlg_packed_agent_size(const MlgAgentDims *d);
int mlg_pack_agent(const MlgAgentDims *d, const MlgAgentParams *p, float *packed, void *stream);

int mlg_env_reset(const MlgEnvSpec *spec, MlgEnvState *st, void *stream);
int mlg_env_step(const MlgEnvSpec *spec, MlgEnvState *st, const int64_t *actions /*[B][N]*/,
                 float *reward /*[B][n_policy_teams]*/, int32_t *done /*[B]*/, int32_t *won /*[B][2]*/,
                 int32_t *draw /*[B]*/, void *stream);
int mlg_env_observe(const MlgEnvSpec *spec, const MlgEnvState *st, float *obs /*[B][N][8U]*/,
                    float *state /*[B][6U]*/, int32_t *avail /*[B][N][A]*/, void *stream);

/* One full ParallelStepper.run: reset all B envs, step until every env terminated, filling `batch`
 * (caller zero-initialised, like EpisodeBatch construction). epsilon already evaluated on the host
 * (DecayThenFlatSchedule.eval(t_env)); test_mode forces epsilon 0. */
int mlg_rollout(const MlgEnvSpec *spec, MlgEnvState *st, const MlgAgentDims *dims, const float *packed,
                MlgBatch *batch, MlgRunInfo *info, float epsilon, int32_t test_mode, void *stream);

/* One full SelfPlayParallelStepper.run: both plan teams are policy-controlled (spec->n_agents = 2 * nh, the
 * first nh agents are the home team). Home agents act with home_packed into `home`, away agents with
 * away_packed into `away` (obs / avail of each side's own agents; state, terminated and filled in both;
 * reward[0] -> home, reward[1] -> away, as stepper_utils.build_pre_transition_data splits them). dims
 * describe ONE side's MAC (n_agents = nh). Epsilon per side; the epsilon RNG stream index is the global
 * agent index (home 0..nh-1, away nh..2nh-1). info->ret_away receives the away returns. */
int mlg_rollout_selfplay(const MlgEnvSpec *spec, MlgEnvState *st, const MlgAgentDims *dims, const float *home_packed,
                         const float *away_packed, MlgBatch *home, MlgBatch *away, MlgRunInfo *info,
                         float eps_home, float eps_away, int32_t test_mode, void *stream);

/* Host only, launches nothing. Writes the name of the kernel mlg_rollout (selfplay = 0) or mlg_rollout_selfplay
 * (selfplay = 1) would launch for this spec and agent dims under the current MLG_ROLLOUT_* environment, and the
 * dynamic LDS bytes of that launch. Names: "v7-static" / "v7" (compile-time 5v5 or 3v3 shape / runtime shape), "v2",
 * "v1-lds/tpwK" / "v1-global/tpwK" (weights in LDS / read from global memory, K agent tiles per wave), "sp8",
 * "sp7-static" / "sp7", "sp2". Both entry points take their decision from the same function. Nonzero
 * (mlg_last_error) where the entry point itself would refuse the shape. */
int mlg_rollout_describe(const MlgEnvSpec *spec, const MlgAgentDims *dims, int32_t selfplay, char *name,
                         int32_t name_cap, int64_t *lds_bytes);

/* Zero `count` EpisodeBatch slots starting at slot0 (mod ring_size) in every key -- one launch; the
 * ring-mode pre-fill that replaces constructing a zero EpisodeBatch. slot_bytes[8] = bytes per slot of
 * state, obs, actions, avail, reward, terminated, actions_onehot, filled. */
int mlg_zero_slots_bytes(const MlgBatch *batch, const int64_t *slot_bytes, int32_t slot0, int32_t count,
                         int32_t ring_size, void *stream);

/* DRQN forward over R rows: q[R][A], h_out[R][H] from inputs[R][d_in], h_in[R][H]. */
int mlg_agent_forward(const MlgAgentDims *d, const float *packed, const float *inputs, const float *h_in,
                      float *q, float *h_out, int32_t R, void *stream);

/* BasicMAC.forward(ep_batch, t): builds inputs from the batch at t (obs, onehot(a_{t-1}), agent id). */
int mlg_mac_forward(const MlgAgentDims *d, const float *packed, const MlgBatch *batch, int32_t t,
                    const float *h_in, float *q /*[B][N][A]*/, float *h_out, void *stream);

/* Epsilon-greedy over rows r of q[R][A] with avail[R][A] (int32). rng key per row:
 * keys[r / n_agents] with ctr(episode[r / n_agents], t, purpose, r % n_agents). */
int mlg_select_actions(const float *q, const int32_t *avail, int32_t R, int32_t A, int32_t n_agents,
                       const uint64_t *keys, const uint32_t *episodes, int32_t t, float epsilon,
                       int64_t *actions, int64_t *is_greedy, void *stream);

/* QMixer forward (hypernet_layers 1 or 2). */
typedef struct {
    const float *hw1_0w, *hw1_0b, *hw1_2w, *hw1_2b; /* hyper_w_1 (2 layers) or hyper_w_1 (1 layer: 0w/0b) */
    const float *hwf_0w, *hwf_0b, *hwf_2w, *hwf_2b;
    const float *hb1_w, *hb1_b;
    const float *v0_w, *v0_b, *v2_w, *v2_b;
    int32_t n_agents, state_dim, embed_dim, hypernet_embed, hypernet_layers;
} MlgQMixParams;
int mlg_qmix_forward(const MlgQMixParams *p, const float *agent_qs /*[R][N]*/, const float *states /*[R][S]*/,
                     float *q_tot /*[R]*/, int32_t R, void *stream);

/* ---- Backward of one agent step / one mixer call (autograd of torch.ops.maleague.drqn_forward / qmix_forward) ----
 * For learners written the reference's way (unroll mac.forward over t, mix, build any loss, loss.backward():
 * src/marl/learners/q_learner.py:47-52,103): PyTorch chains the steps, these entry points differentiate one step.
 * Each recomputes its step's activations from the step's inputs (nothing is kept from the forward), writes row deltas
 * to `workspace` (mlg_*_backward_workspace_floats(dims, R) floats, 16-byte aligned, any contents) and reduces the
 * weight gradients in a fixed order: results are deterministic. dparams is overwritten, not accumulated; R == 0
 * zeroes it. The *_workspace_floats calls are host only and return -1 (message in mlg_last_error()) on bad dims.
 *
 * mlg_agent_backward differentiates DRQNAgentNetwork.forward (src/marl/modules/agents/drqn_agent.py:29-35; torch
 * GRUCell, gates r, z, n). `packed` must be the mlg_pack_agent() block of `p`. h_in NULL = zeros (as the forward),
 * gq [R][A] / gh_out [R][H] NULL = zero upstream gradient, d_inputs [R][d_in] / d_h_in [R][H] NULL = not wanted.
 * dparams: fc1.weight, fc1.bias, gru.weight_ih, gru.weight_hh, gru.bias_ih, gru.bias_hh, fc2.weight, fc2.bias
 * (named_parameters() order, as the learner's flat vectors below). packed, h_in, gh_out, d_h_in 16-byte aligned. */
int64_t mlg_agent_backward_workspace_floats(const MlgAgentDims *d, int32_t R);
int mlg_agent_backward(const MlgAgentDims *d, const MlgAgentParams *p, const float *packed, const float *inputs,
                       const float *h_in, const float *gq, const float *gh_out, float *d_inputs, float *d_h_in,
                       float *dparams, float *workspace, int32_t R, void *stream);
/* mlg_qmix_backward differentiates QMixer.forward (src/marl/modules/mixers/qmix.py:41-59) with respect to agent_qs
 * and every hypernet weight and bias (not the states): g_qtot [R] -> d_agent_qs [R][N]; abs backward is sign with
 * sign(0) = 0, ELU backward 1 for pre > 0 else exp(pre). dparams in named_parameters() order: two layers as the
 * learner's mixer vector below; one layer hyper_w_1.{weight [N*E][S], bias}, hyper_w_final.{weight [E][S], bias},
 * hyper_b_1.{weight, bias}, V.{0.weight, 0.bias, 2.weight, 2.bias}. */
int64_t mlg_qmix_backward_workspace_floats(const MlgQMixParams *p, int32_t R);
int mlg_qmix_backward(const MlgQMixParams *p, const float *agent_qs, const float *states, const float *g_qtot,
                      float *d_agent_qs, float *dparams, float *workspace, int32_t R, void *stream);

/* ---- QLearner.train (q_learner.py:34-131) as one fused device pipeline --------------------------
 * Flat parameter vectors follow the nn.Module named_parameters() order:
 *   agent: fc1.weight [H][d_in], fc1.bias [H], gru.weight_ih [3H][H], gru.weight_hh [3H][H],
 *          gru.bias_ih [3H], gru.bias_hh [3H], fc2.weight [A][H], fc2.bias [A]
 *   qmix (hypernet_layers 2): hyper_w_1.{0.weight [HE][S], 0.bias, 2.weight [N*E][HE], 2.bias},
 *          hyper_w_final.{0.weight [HE][S], 0.bias, 2.weight [E][HE], 2.bias}, hyper_b_1.{weight [E][S], bias},
 *          V.{0.weight [E][S], 0.bias, 2.weight [1][E], 2.bias}
 *   qmix (hypernet_layers 1, the reference QMixer's fallback, qmix.py:17): hyper_w_1.{weight [N*E][S], bias},
 *          hyper_w_final.{weight [E][S], bias}, hyper_b_1.{weight [E][S], bias},
 *          V.{0.weight [E][S], 0.bias, 2.weight [1][E], 2.bias} (the order mlg_qmix_backward documents)
 *   vdn, none (IQL): no mixer parameters, n_mixer = 0: the vectors hold the agent alone
 * params/grads/square_avg = [agent | mixer]; target_params likewise (the target networks).
 * Supported: mixer 0 / 1 / 2; for qmix hypernet_layers 1 or 2, mixing_embed_dim E in {16, 32, 64} and, with two
 * layers, hypernet_embed HE in {32, 64, 128} (one layer ignores HE); N <= 32; H in {32, 64, 128}. Anything else
 * is refused (-1 / nonzero, mlg_last_error() names the key and the supported values).
 * IQL (mixer 0, q_learner.py:55-98 without the mixing): td[b,t,n] = Q_chosen[b,t,n] - (r[b,t] + gamma (1 -
 * term[b,t]) target[b,t+1,n]) with the per-agent double-Q / masked-max target of VDN/QMIX; the mask is expanded
 * over the agents, mask_elems = N sum(mask): loss = sum(mask td^2) / mask_elems, td_error_abs = sum|mask td| /
 * mask_elems, q_taken_mean and target_mean divide by mask_elems * N (the reference's double division, kept).
 * stats[5] = mask_elems, stats[6] = count_nonzero of the expanded mask; trained_steps grows by the latter.
 * agent = 1 (feed-forward, DQNAgentNetwork): the flat agent vector is fc1.weight [H][d_in], fc1.bias [H], fc2.weight
 * [A][H], fc2.bias [A]; H = rnn_hidden_dim is the width of fc1. No recurrence runs: one time-parallel kernel computes
 * relu(fc1) of every live (16-row tile, t) block for the online and the target network, one backward kernel turns the
 * mixer's deltas into the fc1 delta rows, and the workspace holds no GRU buffers. Mask scan, skip rules, mixers, the
 * weight-gradient reduce, clip, RMSprop, target_sync, trained_steps and stats are those of agent = 0; the supported
 * ranges too. A zero-initialised cfg keeps today's meaning.
 * distinct = 1 (one DRQN per agent slot, DistinctMAC): params, grads, square_avg, target_params and target_sync are
 * [agent 0 | agent 1 | ... | agent N-1 | mixer], each agent block in the agent order above with d_in = d_obs (+ A with
 * obs_last_action); mlg_qlearner_param_counts returns n_agent = N x one block. Network n reads the obs / last-action
 * rows of slot n and receives the gradient of slot n's rows only. The agent kernels run N instances of the N = 1, R = B
 * problem selected by a grid coordinate (per-agent strides on the packed weights, the workspace tensors and the
 * gradient output; the weight-gradient jobs repeat per network): the launches per call do not depend on N. Mask scan,
 * skip rules under MLG_LEARNER_FULL, the target pass only when the target differs bitwise, mixers 0 / 1 / 2 at every
 * supported width, double-Q, TD error, stats, the clip over the whole vector, RMSprop, target_sync, host_rows and
 * batch.rows are those of distinct = 0; stats[7] counts the blocks of all N instances, and trained_steps points at N
 * doubles (one per network), each += count_nonzero(mask). Dead-slot rule, decided on the device: a slot to which, in
 * every stored step of the batch (filled != 0), no action other than action 0 is available keeps its chosen Q in the
 * mix, the loss and the statistics, but its network receives an exactly zero gradient in every tensor, is left
 * bit-unchanged by the step, and grad_norm is the norm without its share; a slot alive in any stored step trains on
 * all its rows. Refused by name: agent = 1 with distinct = 1, obs_agent_id = 1, N > 32; H stays in {32, 64, 128}. */
typedef struct {
    int32_t B, T, N, A, d_obs, H, S, E, HE, hypernet_layers;
    int32_t mixer; /* 0 none (IQL), 1 vdn, 2 qmix */
    int32_t double_q, obs_last_action, obs_agent_id;
    float gamma, lr, optim_alpha, optim_eps, grad_norm_clip;
    int32_t agent; /* 0 DRQN (rnn: everything above), 1 feed-forward (dqn): see above */
    int32_t distinct; /* 0 one shared agent, 1 one DRQN per agent slot (mac: distinct): see above */
    int32_t per;      /* 1: prioritized replay (below): the loss weights MlgLearnerBufs.is_weight and the per-episode
                         errors td_abs; 0: neither pointer is read and every launch is the one of the unweighted call */
} MlgLearnerCfg;

typedef struct {
    MlgBatch batch;              /* the truncated sample: B episodes, T = max_t_filled timesteps (batch.T1 = stride) */
    float *params;               /* [n_agent + n_mixer] updated in place (RMSprop) */
    float *grads;                /* [n_agent + n_mixer] out: clipped gradients */
    float *square_avg;           /* [n_agent + n_mixer] RMSprop state */
    const float *target_params;  /* [n_agent + n_mixer] */
    float *workspace;            /* mlg_qlearner_workspace_floats() floats; any contents (a call reads only what it
                                    wrote; one word carries "target differs" between its launches and is cleared
                                    by the last) */
    float *stats;                /* [8] out: loss, grad_norm, td_error_abs, q_taken_mean, target_mean,
                                    mask_sum, count_nonzero(mask), forward (16-row tile, t, net) blocks planned:
                                    sum over tiles of the tile's length, times 2 when the target pass ran
                                    (target_params differ bitwise from params, or MLG_LEARNER_FULL=1) */
    /* optional (NULL = off), folded into the same launches instead of separate copies / adds: */
    float *target_sync;          /* [n_agent + n_mixer] receives the updated parameters (the target update
                                    q_learner.py:127-128 when it is due after this step; usually target_params) */
    double *trained_steps;       /* [1] += count_nonzero(mask) (Agent.trained_steps, q_learner.py:104); distinct = 1:
                                    [N], one per network, each += the same count */
    const int32_t *host_rows;    /* HOST copy of the slot map (B <= 64): travels as a kernel argument,
                                    batch.rows is then ignored */
    /* per = 1 only (prioritized replay): loss = sum_b w_b sum_t (mask td)^2 / sum(mask), so d loss / d q_tot =
     * 2 w_b mtd mask / sum(mask); td_error_abs, q_taken_mean, target_mean, mask_sum and trained_steps stay unweighted.
     * td_abs[b] = sum_t |mask td| / sum_t mask of episode b (IQL: both sums also over the agents; 0 for an episode with
     * no masked step): the TD kernel stores each row's |mask td| and one more small launch adds an episode's rows in a
     * fixed order (no float atomics: the same call gives the same bits). With every weight 1 the parameters, gradients
     * and stats have the bits of the per = 0 call. describe appends " + per"; the workspace grows by B (T - 1) floats. */
    const float *is_weight;      /* [B] importance weights (mlg_per_sample) */
    float *td_abs;               /* [B] out */
} MlgLearnerBufs;

int64_t mlg_qlearner_param_counts(const MlgLearnerCfg *c, int64_t *n_agent, int64_t *n_mixer);
int64_t mlg_qlearner_workspace_floats(const MlgLearnerCfg *c);
/* Largest batch (episodes) whose slot map may travel as MlgLearnerBufs.host_rows (a kernel argument). */
int mlg_qlearner_inline_rows(void);
int mlg_qlearner_train(const MlgLearnerCfg *c, const MlgLearnerBufs *b, void *stream);
/* Host only, launches nothing (the contract of mlg_rollout_describe). Writes the names of the kernels
 * mlg_qlearner_train would launch for this cfg under the current MLG_MIX_GENERIC environment, as
 * "<agent part> + <mixer part>", e.g. "h64/bwd-fused/q1 + qmix-split". mlg_qlearner_train takes its decisions from
 * the same host function. Agent part: h32 | h64 | h128 (the per-H agent kernels), bwd-fused (H = 64: fc2's and the
 * mixer's weight gradients ride in the reverse-recurrence launch, bwd4_wgrad_kernel) or bwd-split, q1..q6 (16-action
 * tiles of agent_q_kernel). Mixer part: iql, vdn-fast / vdn and qmix-split / qmix-generic (default widths E = 32,
 * HE = 64: the prefetching forms up to N = 8, A = 16, S = 64 / the generic mix_td_kernel<64, 32>), qmix1-e{E} (one
 * hypernet layer), qmix-he{HE}-e{E} (the other widths). With agent = 1 the agent part is ff-h32 | ff-h64 | ff-h128 followed by /q1..q6,
 * and QMIX at the default widths runs qmix-generic (no recurrence launch carries the split form). With distinct = 1
 * the agent part is dx-h32 | dx-h64 | dx-h128 followed by /bwd-split/q1..q6 (the <H, true> forms of the agent kernels,
 * prep_kernel<true> and the repeating weight-gradient kernels; the H = 64 fused backward is not carried over), e.g.
 * "dx-h64/bwd-split/q1 + qmix-generic"; the mixer part is iql, vdn-fast / vdn, qmix-generic, qmix1-e{E} or
 * qmix-he{HE}-e{E} (no qmix-split: the hypernet tiles ride in the shared agent's recurrence launch only). With per = 1
 * " + per" follows the mixer part (the PER form of the same TD kernel and the per-episode reduce). Nonzero
 * (mlg_last_error) where mlg_qlearner_train would refuse the cfg. */
int mlg_qlearner_describe(const MlgLearnerCfg *c, char *name, int32_t name_cap);


/* ---- REFIL (config 5): entity scheme, EntityAttentionRNNAgent, FlexQMixer, REFILLearner ----------------- */
/* Entity env variant: base.U = 2S units, policy team 0 = units 0..S-1 (= the agents = entities
 * 0..S-1), scripted team 1 = S..2S-1; per episode k ~ U{min_agents..max_agents} active slots per team. */
typedef struct {
    MlgEnvSpec base;
    int32_t min_agents, max_agents;
} MlgEntityEnvSpec;

/* Entity-scheme EpisodeBatch, all [B][T1][...] row-major (REFIL scheme: no state / obs). */
typedef struct {
    float *entities;       /* [B][T1][NE][ED] */
    uint8_t *obs_mask;     /* [B][T1][NE][NE]  1 = entity not observable by the row entity */
    uint8_t *entity_mask;  /* [B][T1][NE]      1 = entity absent (padding) or dead */
    int64_t *actions;      /* [B][T1][NA][1] */
    int32_t *avail;        /* [B][T1][NA][A] */
    float *reward;         /* [B][T1][1] */
    uint8_t *terminated;   /* [B][T1][1] */
    float *actions_onehot; /* [B][T1][NA][A] */
    int64_t *filled;       /* [B][T1][1] */
    int32_t B, T1, ring_slot0, ring_size, full_write; /* as MlgBatch */
    const int32_t *rows;   /* sampled view (learner): episode b lives in slot rows[b]; nullptr = identity */
    int32_t *slot_extent;  /* as MlgBatch */
} MlgEntityBatch;

typedef struct {
    int32_t n_agents, n_entities, entity_shape, n_actions, entity_last_action;
    int32_t attn_embed_dim, attn_n_heads, rnn_hidden_dim;
} MlgRefilDims;

/* Packed EntityAttentionRNNAgent weights from the flat named_parameters() vector: fc1.weight [64][D0], fc1.bias,
 * attn.in_trans.weight [192][64], attn.out_trans.weight [64][64], attn.out_trans.bias, fc2.weight, fc2.bias,
 * rnn.weight_ih [192][64], rnn.weight_hh, rnn.bias_ih [192], rnn.bias_hh, fc3.weight [A][64], fc3.bias
 * (D0 = entity_shape + n_actions with entity_last_action). */
int64_t mlg_refil_packed_agent_size(const MlgRefilDims *d);
int mlg_refil_pack_agent(const MlgRefilDims *d, const float *flat, float *packed, void *stream);

/* One EntityAttentionRNNAgent.forward step (ts = 1) over R items: entities [R][NE][D0] (last-action one-hot
 * included), obs_mask [R][NE][NE], entity_mask [R][NE], h_in [R][NA][64] -> q [R][NA][A], h_out [R][NA][64]. */
int mlg_refil_agent_forward(const MlgRefilDims *d, const float *packed, const float *entities, const uint8_t *obs_mask,
                            const uint8_t *entity_mask, const float *h_in, float *q, float *h_out, int32_t R,
                            void *stream);

/* One ParallelStepper.run over the entity env with EntityMAC acting (entity_controller.py:11-30 with
 * t -> slice(t, t + 1); entity_rnn_agent.py:32-65; action_selectors.py:44-62). Same run semantics, ring /
 * full-write modes and run info as mlg_rollout. */
int mlg_refil_rollout(const MlgEntityEnvSpec *spec, MlgEnvState *st, const MlgRefilDims *d, const float *packed,
                      MlgEntityBatch *batch, MlgRunInfo *info, float epsilon, int32_t test_mode, void *stream);

/* Host only, launches nothing (the contract of mlg_rollout_describe). Writes the name of the kernel mlg_refil_rollout
 * would launch for this spec and agent dims under the current MLG_REFIL_ROLLOUT / MLG_REFIL_GENERIC environment, and
 * the dynamic LDS bytes of that launch. Names: "ro4-static" / "ro4" (four envs per wave: the compile-time refil_8
 * shape / runtime shape), "ro2/kc1", "ro2/kc2", "ro2/kc3" (two envs per wave, entity input width 16 / 32 / 48).
 * mlg_refil_rollout takes its decision from the same function. Nonzero (mlg_last_error) where it would refuse the
 * shape. */
int mlg_refil_rollout_describe(const MlgEntityEnvSpec *spec, const MlgRefilDims *d, char *name, int32_t name_cap,
                               int64_t *lds_bytes);

/* One SelfPlayParallelStepper.run over the two-policy entity env (DESIGN.md §3b'): both teams are policy-controlled
 * (spec->base: n_policy_teams = 2, scripted = [0, 0], n_agents = 2S, agent_unit[a] = a; home = units 0..S-1, away =
 * units S..2S-1), an EntityMAC on each side. `d` describes ONE side (n_agents = S, n_entities = 2S); both packed blocks
 * are mlg_refil_pack_agent's, 16-byte aligned. The home batch is what mlg_refil_rollout records (raw unit order and
 * action indices, team 0's reward). The away batch holds the same state in the canonical view: entity j' = unit
 * (j' + S) mod 2S, x mirrored to G - 1 - x, team flipped, obs_mask / entity_mask permuted the same way, actions 3 / 4
 * swapped and target 5 + j' = raw target 5 + (j' + S) mod 2S in avail, actions, actions_onehot and the last-action
 * columns; team 1's reward; terminated / filled as home. The env executes the raw image of the away choice (an
 * unavailable choice is a no-op). Epsilon per side, RNG stream index = global agent index (home n, away S + n); the
 * random action is the k-th available in the side's own index order. One launch, no host wait. Each batch honours
 * ring_slot0 / ring_size / full_write / slot_extent on its own. info->ret / ret_away = the two returns, won[2b] = home;
 * agent_rows counts both sides. entity_last_action may be 0 (no last-action columns). */
int mlg_refil_rollout_selfplay(const MlgEntityEnvSpec *spec, MlgEnvState *st, const MlgRefilDims *d,
                               const float *home_packed, const float *away_packed, MlgEntityBatch *home,
                               MlgEntityBatch *away, MlgRunInfo *info, float eps_home, float eps_away,
                               int32_t test_mode, void *stream);
/* Host only, launches nothing (the contract of mlg_refil_rollout_describe). Names: "sp-ro2/kc1", "sp-ro2/kc2",
 * "sp-ro2/kc3" (two envs per wave, both sides' agent phases per step; entity input width 16 / 32 / 48).
 * mlg_refil_rollout_selfplay takes its decision from the same function. Nonzero (mlg_last_error) where it would refuse
 * the spec or dims. */
int mlg_refil_rollout_selfplay_describe(const MlgEntityEnvSpec *spec, const MlgRefilDims *d, char *name,
                                        int32_t name_cap, int64_t *lds_bytes);

/* EntityAttentionLayer.forward (src/marl/modules/layers/attention.py:24-79; in = embed = out = 64, 4 heads) over bs
 * items: x [bs][ne][64], pre_mask [bs][nq][ne], post_mask [bs][nq] (uint8, 1 = masked) -> y [bs][nq][64]. Forward
 * only: its backward is mlg_refil_attention_backward below. */
int mlg_refil_attention(const float *w_in, const float *w_out, const float *b_out, const float *x,
                        const uint8_t *pre_mask, const uint8_t *post_mask, int32_t bs, int32_t ne, int32_t nq,
                        int32_t n_heads, float *y, void *stream);

/* FlexQMixer (flex_qmix.py:55-117): packed = 4 AttentionHyperNet blocks from the flat named_parameters() vector
 * (hyper_w_1, hyper_w_final, hyper_b_1, V); forward over R rows: agent_qs [R][NA] (plain) or [R][2 NA] with the
 * imagine masks w_mask / i_mask [R][NE][NE] (both or neither), entities [R][NE][D0], entity_mask [R][NE]
 * -> q_tot [R]. softmax_mixing_weights selects softmax instead of abs mixing weights. */
int64_t mlg_refil_packed_mixer_size(const MlgRefilDims *d);
int mlg_refil_pack_mixer(const MlgRefilDims *d, const float *flat, float *packed, void *stream);
int mlg_refil_mixer_forward(const MlgRefilDims *d, const float *packed, const float *agent_qs, const float *entities,
                            const uint8_t *entity_mask, const uint8_t *w_mask, const uint8_t *i_mask,
                            int32_t softmax_mixing_weights, float *q_tot, int32_t R, void *stream);

/* ---- Backward of the REFIL layer ops (autograd of torch.ops.maleague.refil_attention / entity_agent_forward) ----
 * For REFIL learners written the reference's way (src/marl/learners/refil_learner.py:102-218: unroll the MAC, gather,
 * build a loss, loss.backward()). Same contract as mlg_agent_backward above: each call recomputes its forward from the
 * step's inputs, writes row activations and deltas to `workspace` (*_workspace_floats floats, 16-byte aligned, any
 * contents) and reduces every weight and bias gradient in a fixed order (no float atomics: bitwise reproducible).
 * dparams is overwritten; bs == 0 / R == 0 zeroes it and launches nothing. Entities and masks get no gradient. The
 * *_workspace_floats calls are host only and return -1 (message in mlg_last_error()) on bad dims.
 *
 * mlg_refil_attention_backward differentiates EntityAttentionLayer.forward (src/marl/modules/layers/attention.py:24-79;
 * shapes as mlg_refil_attention): gy [bs][nq][64] -> dx [bs][ne][64] and dparams = in_trans.weight [192][64],
 * out_trans.weight [64][64], out_trans.bias [64]. Post-masked query rows pass no gradient; a query row whose every key
 * is pre-masked contributes zero (attention.py:59). workspace, w_in, w_out and dx 16-byte aligned. */
int64_t mlg_refil_attention_backward_workspace_floats(int32_t bs, int32_t ne, int32_t nq, int32_t n_heads);
int mlg_refil_attention_backward(const float *w_in, const float *w_out, const float *b_out, const float *x,
                                 const uint8_t *pre_mask, const uint8_t *post_mask, const float *gy, int32_t bs,
                                 int32_t ne, int32_t nq, int32_t n_heads, float *dx, float *dparams, float *workspace,
                                 void *stream);
/* mlg_refil_mixer_backward differentiates FlexQMixer.forward (src/marl/modules/mixers/flex_qmix.py:73-117; inputs as
 * mlg_refil_mixer_forward, `packed` the mlg_refil_pack_mixer() block of the parameters), plain or with imagine groups,
 * abs or softmax mixing weights: g_qtot [R] -> d_agent_qs (the shape of agent_qs) and dparams, the 4 x 7 hypernet
 * parameters in the flat order of mlg_refil_pack_mixer. `imagine` of the workspace query: nonzero when the call passes
 * w_mask / i_mask. workspace and packed 16-byte aligned. */
int64_t mlg_refil_mixer_backward_workspace_floats(const MlgRefilDims *d, int32_t R, int32_t imagine);
int mlg_refil_mixer_backward(const MlgRefilDims *d, const float *packed, const float *agent_qs, const float *entities,
                             const uint8_t *entity_mask, const uint8_t *w_mask, const uint8_t *i_mask,
                             int32_t softmax_mixing_weights, const float *g_qtot, float *d_agent_qs, float *dparams,
                             float *workspace, int32_t R, void *stream);
/* mlg_refil_agent_backward differentiates one EntityAttentionRNNAgent.forward step
 * (src/marl/modules/agents/entity_rnn_agent.py:32-65; inputs as mlg_refil_agent_forward, `packed` the
 * mlg_refil_pack_agent() block of the parameters): gq [R][NA][A] / gh_out [R][NA][64] (NULL = zero upstream gradient)
 * -> d_h_in [R][NA][64] (NULL = not wanted) and dparams, the 13 parameters in the flat order of mlg_refil_pack_agent.
 * q of an entity-masked agent is 0, so its gq row reaches nothing; its GRU still runs, so its gh_out row reaches h_in,
 * fc2.bias and the GRU weights. workspace, packed, h_in, gh_out and d_h_in 16-byte aligned. */
int64_t mlg_refil_agent_backward_workspace_floats(const MlgRefilDims *d, int32_t R);
int mlg_refil_agent_backward(const MlgRefilDims *d, const float *packed, const float *entities,
                             const uint8_t *obs_mask, const uint8_t *entity_mask, const float *h_in, const float *gq,
                             const float *gh_out, float *d_h_in, float *dparams, float *workspace, int32_t R,
                             void *stream);

/* REFILLearner.train (src/marl/learners/refil_learner.py:102-218) as one device pipeline: EntityMAC unrolls of the
 * plain / within / interact copies + target, FlexQMixer (flex_qmix.py:55-117) plain + imagined mixing, double-Q
 * targets, the lambda-mixed TD loss, all gradients, clip_grad_norm_ and RMSprop.
 * Flat parameters = [agent | mixer]; agent in named_parameters order (see mlg_refil_pack_agent); mixer =
 * hyper_w_1, hyper_w_final, hyper_b_1, V, each: fc1.weight [64][D0], fc1.bias, attn.in_trans.weight [192][64],
 * attn.out_trans.weight [64][64], attn.out_trans.bias, fc2.weight [32][64], fc2.bias [32]. */
typedef struct {
    int32_t B, T, n_agents, n_entities, entity_shape, n_actions, entity_last_action;
    int32_t attn_embed_dim, attn_n_heads, rnn_hidden_dim, hypernet_embed, mixing_embed_dim;
    int32_t double_q, softmax_mixing_weights;
    int32_t imagine; /* 1: imagine_entity_attend_rnn (REFIL: plain + within + interact copies, the lambda-mixed loss);
                        0: entity_attend_rnn (one online copy, the masked TD loss alone; groupA may be NULL and is
                        never read, stats[1] = 0) */
    int32_t mixer;   /* 0: flex_qmix; 1: vdn (imagine = 0 only): q_tot = sum of the chosen Q over the agents, the
                        flat parameters are the agent alone (n_mixer = 0) and no hypernet kernel runs */
    float gamma, lmbda, lr, optim_alpha, optim_eps, grad_norm_clip;
} MlgRefilLearnerCfg;

typedef struct {
    MlgEntityBatch batch;        /* B episodes, T timesteps used (batch.T1 = stride) */
    const uint8_t *groupA;       /* [B][NE] the imagine group draw per episode (entity_rnn_agent.py:95-97) */
    float *params;               /* [n_agent + n_mixer] updated in place (RMSprop) */
    float *grads;                /* [n_agent + n_mixer] out: clipped gradients */
    float *square_avg;           /* RMSprop state */
    const float *target_params;  /* target networks, same layout */
    float *workspace;            /* mlg_refil_workspace_floats() floats */
    float *stats;                /* [8] out: loss, im_loss, grad_norm, td_error_abs, q_taken_mean, target_mean,
                                    mask_sum, 0 */
    double *trained_steps;       /* optional [1] += mask_sum (Agent.trained_steps, refil_learner.py:176) */
    float *target_sync;          /* optional (NULL = off) [n_agent + n_mixer] receives the updated parameters in the
                                    optimizer launch: the target update when due after this step
                                    (refil_learner.py:181-183 -> _update_targets; usually target_params) */
    const int32_t *host_rows;    /* optional (NULL = off) HOST copy of the slot map (B <= mlg_qlearner_inline_rows()):
                                    travels as a kernel argument, batch.rows is then ignored */
} MlgRefilLearnerBufs;

int64_t mlg_refil_param_counts(const MlgRefilLearnerCfg *c, int64_t *n_agent, int64_t *n_mixer);
int64_t mlg_refil_workspace_floats(const MlgRefilLearnerCfg *c);
int mlg_refil_train(const MlgRefilLearnerCfg *c, const MlgRefilLearnerBufs *b, void *stream);
/* The imagine group draw of a train call (entity_rnn_agent.py:95-97: p_b = rand per episode, groupA[b][j] =
 * bernoulli(p_b)) on the device, counter-based from (seed, draw): one launch into groupA [B][NE]. */
int mlg_refil_draw_groups(int32_t B, int32_t NE, uint64_t seed, uint32_t draw, uint8_t *groupA, void *stream);

/* Diagnostic builds only (-DMLG_STAMPS): device buffer [grid][8 waves][16] u64 of per-phase cycle counts
 * of mlg_rollout. Returns nonzero in normal builds. */
int mlg_debug_set_stamps(void *ptr);
/* Diagnostic builds only (-DMLG_STAMPS): per-wave phase cycle counters of the learner recurrences. */
int mlg_debug_set_learner_stamps(void *ptr);
int mlg_refil_debug_set_stamps(void *ptr); /* same for mlg_refil_rollout: [grid][16] u64 */

/* League payoff bookkeeping of one batched self-play run (league_experiment_process.py:85-105, _extract_result +
 * _update_payoff per env): entry = the league's local payoff delta [GAMES, WIN, LOSS, DRAW, ...] of (home, away);
 * won [B][2] (policy team first), draw [B] as written by mlg_rollout_selfplay. DRAW if draw or both / no team won,
 * else WIN / LOSS by won[b][0]; GAMES += B when count_games (the reference never counts GAMES). One launch. */
int mlg_league_record_runs(const int32_t *won, const int32_t *draw, int32_t B, float *entry, int32_t count_games,
                           void *stream);

/* ---- Cross-play evaluation (joint-policy correlation, src/runs/evaluation/jpc_eval_run.py:62-89): every
 * (home policy, away policy, roster) pair of a league pool in ONE greedy rollout launch that writes no EpisodeBatch.
 * Pair k plays E episodes; env (k, e) runs exactly as env index e with episode counter episode0 of a test-mode
 * mlg_rollout_selfplay under specs[pair.spec] (key mlg_env_key(seed, e), counters mlg_ctr(episode0, t, ..)): every
 * pair sees the same E spawn draws, no MlgEnvState is read or advanced, and the per-env results are bit-identical to
 * that self-play run on the fp32 (v1) kernel. A workgroup owns 16 envs of one pair (grid n_pairs * ceil(E / 16)) and
 * reads its two policies from packed_pool by index. The obs / avail rows of the current step stay in LDS; when the
 * one-step obs of 16 envs does not fit (or MLG_CROSSPLAY_OBS_WORKSPACE=1) they live in `workspace`, one step per
 * workgroup. Nothing scales with episode_limit. */
typedef struct {
    int32_t home, away; /* rows of packed_pool */
    int32_t spec;       /* index into specs */
} MlgCrossplayPair;

typedef struct {
    const float *packed_pool;           /* device [n_pool][mlg_packed_agent_size(dims)], 16-byte aligned */
    int32_t n_pool;
    int32_t n_pairs;
    const MlgCrossplayPair *pairs;      /* device [n_pairs]: what the launch reads (uploaded by the caller) */
    const MlgCrossplayPair *host_pairs; /* HOST copy of the same table: validated (indices in range), never launched */
    const MlgEnvSpec *specs;            /* device [n_specs]: what the launch reads */
    const MlgEnvSpec *host_specs;       /* HOST copy: each a valid two-policy-team spec; all agree on U, n_agents,
                                           n_actions, grid, episode_limit, stochastic, policy_team and seed (team /
                                           role / melee / agent_unit may differ: composed rosters) */
    int32_t n_specs;
    int32_t E;                          /* episodes per pair (any E >= 1) */
    uint32_t episode0;
    float *workspace;                   /* mlg_crossplay_workspace_floats() floats, 16-byte aligned, any contents */
    int64_t workspace_floats;           /* floats `workspace` holds (checked against what the launch needs) */
    /* per-env results [n_pairs * E], semantics of MlgRunInfo after mlg_rollout_selfplay */
    int32_t *ep_len;
    float *ret, *ret_away;
    int32_t *won;                       /* [n_pairs * E][2], home first */
    int32_t *draw;
    /* [n_pairs][8]: games, home wins, away wins, draws, sum ret home, sum ret away, sum ep_len, 0. Win / loss / draw
     * as mlg_league_record_runs (draw if the env says so or both / neither won). Reduced by a second kernel of the same
     * call in a fixed order (bitwise reproducible, no atomics): lane l of 64 adds the envs e = l, l + 64, ... in
     * ascending order starting from 0, then the 64 partial sums are added in ascending lane order starting from 0. */
    float *summary;
} MlgCrossplay;

/* dims describe ONE side's MAC, as for mlg_rollout_selfplay. Host only; -1 (mlg_last_error()) on bad dims. */
int64_t mlg_crossplay_workspace_floats(const MlgAgentDims *dims, int32_t n_pairs, int32_t E);
int mlg_crossplay_rollout(const MlgAgentDims *dims, const MlgCrossplay *c, void *stream);

/* Packs P flat agent parameter rows (named_parameters() order: fc1.weight, fc1.bias, gru.weight_ih, gru.weight_hh,
 * gru.bias_ih, gru.bias_hh, fc2.weight, fc2.bias; row p at flat + p * row_stride floats) into packed_pool
 * [P][mlg_packed_agent_size(dims)]; each row equals mlg_pack_agent() of the same parameters. One launch. */
int mlg_pack_agent_pool(const MlgAgentDims *dims, const float *flat, int64_t row_stride, int32_t P,
                        float *packed_pool, void *stream);

/* ---- Self-play against an opponent mixture (league matches): one away policy and roster per 16 envs -------------
 * Env b belongs to group g = b / 16; n_groups = ceil(B / 16). Group g plays the home policy against away policy
 * packed_pool[groups[g].away] (a row written by mlg_pack_agent_pool) under the roster specs[groups[g].spec]. Env b
 * runs EXACTLY as env b of mlg_rollout_selfplay from the same MlgEnvState with that away block and that spec: the same
 * home weights and epsilons (one away epsilon for every opponent), RNG key mlg_env_key(seed, b), counters and stream
 * index (the global agent index), ring / full-write / slot_extent modes. Its rows of both batches and its run info
 * are bit-identical to that plain launch on the same arm family (a row of an MFMA tile depends on its own inputs only).
 * Host copies are validated before anything is launched and are never launched themselves; the kernels read the device
 * copies and guard the indices they read: a group whose device row is out of range plays nothing (ep_len -1, returns
 * 0, won / draw 0, no batch row written). */
typedef struct {
    int32_t away; /* row of packed_pool */
    int32_t spec; /* index into specs */
} MlgMixGroup;

typedef struct {
    const float *packed_pool;      /* device [n_pool][mlg_packed_agent_size(dims)], 16-byte aligned */
    int32_t n_pool;
    int32_t n_groups;              /* ceil(B / 16) */
    const MlgMixGroup *groups;     /* device [n_groups]: what the launch reads */
    const MlgMixGroup *host_groups; /* HOST copy: validated (indices in range), never launched */
    const MlgEnvSpec *specs;       /* device [n_specs]: what the launch reads */
    const MlgEnvSpec *host_specs;  /* HOST copy: valid two-policy-team specs that agree with each other and with spec0 on
                                      U, n_agents, n_actions, grid, episode_limit, stochastic, policy_team and seed
                                      (team / role / melee / agent_unit may differ: composed rosters); agents 0..nh-1
                                      are the home team in each */
    int32_t n_specs;
} MlgOpponentMix;

/* mlg_rollout_selfplay's arguments with the away policy and the roster taken per group from `mix`; spec0 gives the
 * shape every spec shares (host_specs[k] must agree with it). Two arms: "sp8-mix" exactly when mlg_rollout_selfplay
 * would launch "sp8" for the shape (static 5v5 / 3v3 plans at H = 64; one group per sp8 workgroup), else "v1-mix/tpwK",
 * the generic fp32 self-play kernel with global-memory weights (MLG_ROLLOUT_KERNEL=v1 | sp2 | sp7 and
 * MLG_ROLLOUT_GENERIC included: sp7 / sp2 have no mixture form). One launch. */
int mlg_rollout_selfplay_mix(const MlgEnvSpec *spec0, MlgEnvState *st, const MlgAgentDims *dims,
                             const float *home_packed, const MlgOpponentMix *mix, MlgBatch *home, MlgBatch *away,
                             MlgRunInfo *info, float eps_home, float eps_away, int32_t test_mode, void *stream);
/* Host only, launches nothing (the contract of mlg_rollout_describe): the arm mlg_rollout_selfplay_mix would launch for
 * this shape under the current MLG_ROLLOUT_* environment and its dynamic LDS bytes. */
int mlg_rollout_selfplay_mix_describe(const MlgEnvSpec *spec0, const MlgAgentDims *dims, char *name, int32_t name_cap,
                                      int64_t *lds_bytes);

/* mlg_league_record_runs per opponent: env b books into row + group_col[b / 16] * entry_stride (a payoff entry
 * [GAMES, WIN, LOSS, DRAW, ...]) by the same win / loss / draw rule; GAMES += the column's envs when count_games.
 * group_col: device [ceil(B / 16)], each in [0, n_cols) (a group whose column is out of range books nothing); equal
 * columns add up. Integer counts, reduced in a fixed order (wave w of the one workgroup owns the columns w, w + 16,
 * ...; lane l counts the envs l, l + 64, ... of every group of the column in ascending order, then the 64 lane counts
 * are added by an integer butterfly), no float atomics. One launch. */
int mlg_league_record_runs_mix(const int32_t *won, const int32_t *draw, int32_t B, const int32_t *group_col,
                               int32_t n_cols, float *row, int64_t entry_stride, int32_t count_games, void *stream);

/* ---- COMA (algs/coma.yaml): policy output, multinomial selection, critic training, actor loss ------------- */
/* MultiAgentController._softmax (multi_agent_controller.py:78-99) over R rows of logits [R][A] with avail [R][A]:
 * with mask_before_softmax unavailable logits count as -1e10 in a max-subtracted fp32 softmax; unless test_mode the
 * epsilon floor (1 - eps) p + eps / K follows, K = the row's available actions with masking, else A, and with masking
 * unavailable entries are then 0 (a row with no available action is all 0, never NaN; in test mode the reference
 * zeroes nothing and such a row is the softmax's 1 / A). The backward gives d logits from g_probs [R][A]; the masked
 * assignments pass no gradient. */
int mlg_policy_probs(const float *logits, const int32_t *avail, int32_t R, int32_t A, float epsilon,
                     int32_t mask_before_softmax, int32_t test_mode, float *probs, void *stream);
int mlg_policy_probs_backward(const float *logits, const int32_t *avail, const float *g_probs, int32_t R, int32_t A,
                              float epsilon, int32_t mask_before_softmax, int32_t test_mode, float *d_logits,
                              void *stream);

/* MultinomialActionSelector.select (action_selectors.py:11-32) with this project's counter RNG instead of torch's
 * generator: m_k = probs_k where available, else 0; total = the fp32 sum of m_k in ascending k;
 * u = mlg_u01(mlg_rng(keys[r / n_agents], mlg_ctr(episodes[r / n_agents], t, MLG_PURPOSE_POLICY = 5, r % n_agents)));
 * the action is the first available k whose running fp32 sum exceeds u * total, else the last available k. greedy
 * (test_mode and test_greedy): the first available k with the largest m_k. A row with no available action gets 0. */
int mlg_select_multinomial(const float *probs, const int32_t *avail, int32_t R, int32_t A, int32_t n_agents,
                           const uint64_t *keys, const uint32_t *episodes, int32_t t, int32_t greedy,
                           int64_t *actions, void *stream);

/* One full ParallelStepper.run with a pi_logits MAC (BasicMAC.select_actions, basic_controller.py:29-50, with
 * agent_output_type "pi_logits" and the multinomial selector): mlg_rollout's arguments, run semantics, ring and
 * full-write modes and MlgRunInfo, on the generic fp32 rollout kernel (H in {32, 64, 128}); per step the agent's
 * outputs go through the mlg_policy_probs rule (epsilon is the selector's, test_mode drops the floor) and the action
 * is drawn by the mlg_select_multinomial rule with key mlg_env_key(seed, env), the env's episode counter, the step t
 * and the agent index; test_mode with test_greedy takes the first-index argmax. One launch. The sums of a row add each
 * lane's four actions first, then the four lanes in ascending order, then the 16-action tiles in ascending order (the
 * stand-alone entry points add in ascending k): probabilities agree to rounding, not bitwise. */
int mlg_rollout_policy(const MlgEnvSpec *spec, MlgEnvState *st, const MlgAgentDims *dims, const float *packed,
                       MlgBatch *batch, MlgRunInfo *info, float epsilon, int32_t test_mode,
                       int32_t mask_before_softmax, int32_t test_greedy, void *stream);

/* Host only, launches nothing (the contract of mlg_rollout_describe). Writes the name of the instantiation
 * mlg_rollout_policy would launch for this spec and agent dims, and the dynamic LDS bytes of that launch. Names:
 * "policy-lds/tpwK" / "policy-global/tpwK" (the policy's weights in LDS / read from global memory, K = 1..4 agent tiles
 * per wave). mlg_rollout_policy takes its decision from the same function. Nonzero (mlg_last_error) where it would
 * refuse the spec or the dims. */
int mlg_rollout_policy_describe(const MlgEnvSpec *spec, const MlgAgentDims *dims, char *name, int32_t name_cap,
                                int64_t *lds_bytes);

/* One full SelfPlayPolicyParallelStepper.run: two pi_logits MACs in one launch. The arguments of mlg_rollout_selfplay
 * plus mask_before_softmax and test_greedy (one value for both sides). Semantics: mlg_rollout_selfplay on the generic
 * fp32 arm with the selection site of mlg_rollout_policy on both sides. Side s (0 home, 1 away) uses its own weights
 * and its own epsilon floor (eps_home / eps_away; zero in test mode). Agent a = s * nh + ln of env b draws
 * mlg_u01(mlg_rng(mlg_env_key(seed, b), mlg_ctr(episode, t, MLG_PURPOSE_POLICY, a))). Each side is recorded into its
 * own batch as a test-mode pick (the floor is in the probabilities: no epsilon-greedy redraw). reward[0] / reward[1],
 * ret_away and the ring / full-write / slot_extent modes are mlg_rollout_selfplay's. Refuses, through mlg_last_error
 * and without launching, more than 16 agents per side (2 nh tiles over at most 8 waves, at most 4 per wave), hidden
 * widths other than 32 / 64 / 128 and n_actions beyond five 16-wide action tiles. One launch. */
int mlg_rollout_selfplay_policy(const MlgEnvSpec *spec, MlgEnvState *st, const MlgAgentDims *dims,
                                const float *home_packed, const float *away_packed, MlgBatch *home, MlgBatch *away,
                                MlgRunInfo *info, float eps_home, float eps_away, int32_t test_mode,
                                int32_t mask_before_softmax, int32_t test_greedy, void *stream);

/* Host only, launches nothing (the contract of mlg_rollout_describe). Names: "sp-policy-lds/tpwK" (both sides' weight
 * images staged in LDS: when both fit beside the env state, H = 32) / "sp-policy-global/tpwK" (weights read from global
 * memory; MLG_ROLLOUT_GLOBAL_WEIGHTS forces it), K = 1..4 agent tiles per wave. mlg_rollout_selfplay_policy takes its
 * decision from the same function. Nonzero (mlg_last_error) where it would refuse the spec or the dims. */
int mlg_rollout_selfplay_policy_describe(const MlgEnvSpec *spec, const MlgAgentDims *dims, char *name,
                                         int32_t name_cap, int64_t *lds_bytes);

/* mlg_crossplay_rollout for pi_logits policies: the same MlgCrossplay block, checks, outputs and summary; the pick is
 * mlg_rollout_policy's in test mode. test_greedy = 1: the first-index argmax of the masked probabilities; 0: a draw
 * from the floor-less probabilities on the counter RNG above with c->episode0 as the episode counter. The per-env
 * results of pair k are bit-identical to one test-mode mlg_rollout_selfplay_policy launch of that pair (env index e,
 * episode counter episode0) on the global arm. */
int mlg_crossplay_rollout_policy(const MlgAgentDims *dims, const MlgCrossplay *c, int32_t mask_before_softmax,
                                 int32_t test_greedy, void *stream);

/* The COMA actor loss (coma_learner.py:75-96), forward and d loss / d pi in one launch. rows = B (T - 1) mask entries,
 * pi / avail / q_vals [rows][N][A], actions [rows][N], mask [rows]: pi is zeroed where unavailable and renormalised,
 * baseline = sum pi q, advantage = q_taken - baseline (a constant for the gradient), pi_taken = 1 where mask == 0,
 * loss = -sum(log pi_taken * advantage * mask) / (N sum mask). out[4] = loss, advantage_mean, the masked mean of max
 * pi, N sum mask. d_pi [rows][N][A]; an all-unavailable (padding) row has pi = 0 and zero gradient. One workgroup,
 * every sum in a fixed order. */
int mlg_coma_policy_loss(const float *pi, const int32_t *avail, const int64_t *actions, const float *q_vals,
                         const float *mask, int32_t rows, int32_t N, int32_t A, float *out, float *d_pi,
                         void *stream);

/* COMALearner._train_critic (coma_learner.py:121-169) with COMACritic (critics/coma.py:22-73) and
 * build_td_lambda_targets (coma_learner.py:10-21) as one queued chain of launches without a host wait.
 * Flat critic parameters in named_parameters() order: fc1.weight [128][D], fc1.bias, fc2.weight [128][128], fc2.bias,
 * fc3.weight [A][128], fc3.bias; D = S + d_obs + 2 N A + N. Input row (b, t, n), built in the kernels from the batch
 * (rows honoured): [state | obs_n | actions_onehot at t with agent n's block zeroed | actions_onehot at t - 1 (zeros
 * at t = 0) | eye row n]. One call: the target critic over all T steps with the taken targets gathered; the TD(lambda)
 * recursion; then for t = T - 2 .. 0 one optimizer step (forward at t with the current parameters -> q_vals[:, t],
 * masked MSE over mask_t expanded to the agents, backward, clip_grad_norm_, RMSprop with lr; no momentum, not
 * centered), skipped on the device when sum_b mask[b, t] == 0 (q_vals[:, t] = 0). Three launches per step; every
 * reduction in a fixed order without float atomics: the same inputs give the same bits.
 * Supported: hidden 128, N <= 32, A <= 96; anything else is refused, mlg_last_error() names the key. */
typedef struct {
    int32_t B, T, N, A, d_obs, S, hidden;
    float lr, optim_eps, grad_norm_clip; /* critic_lr, RMSprop eps, clip */
    /* doubles, as the reference holds them: lambda gamma, (1 - lambda) gamma and 1 - alpha are formed in double and
     * rounded to fp32 once, as torch rounds the Python floats it is handed (1.f - 0.99f is not fp32(0.01)) */
    double gamma, td_lambda, optim_alpha;
} MlgComaCfg;

typedef struct {
    MlgBatch batch;             /* B episodes, T timesteps used (batch.T1 = stride) */
    float *params;              /* [n] updated in place */
    float *grads;               /* [n] out: the clipped gradients of the last taken step */
    float *square_avg;          /* [n] RMSprop state */
    const float *target_params; /* [n] the target critic */
    float *workspace;           /* mlg_coma_workspace_floats() floats, any contents */
    float *q_vals;              /* [B][T-1][N][A] out */
    float *targets;             /* [B][T-1][N] out: the TD(lambda) targets */
    float *stats;               /* [6] out: sums over the taken steps of loss, grad_norm, td_error_abs, q_taken_mean,
                                   target_mean; the number of taken steps */
    int64_t *counters;          /* [2] critic_training_steps (+= taken steps), last_target_update_step */
} MlgComaBufs;

int64_t mlg_coma_param_count(const MlgComaCfg *c);     /* host only; -1 (mlg_last_error()) on unsupported dims */
int64_t mlg_coma_workspace_floats(const MlgComaCfg *c); /* host only; -1 likewise */
int mlg_coma_critic_train(const MlgComaCfg *c, const MlgComaBufs *b, void *stream);
/* coma_learner.py:104-106 on the device: when (counters[0] - counters[1]) / interval >= 1, target_params = params and
 * counters[1] = counters[0]. Two launches, no host sync. */
int mlg_coma_target_update(const float *params, float *target_params, int64_t n, int64_t *counters, int32_t interval,
                           void *stream);

/* ---- Feed-forward agent (agent: dqn): q = fc2(relu(fc1(inputs))), no recurrence ------------------------------
 * DQNAgentNetwork (src/marl/modules/agents/dqn_agent.py:9-37); MlgAgentDims as for the DRQN, hidden = rnn_hidden_dim
 * (the width of fc1), H in {32, 64, 128}. Canonical nn.Module layout (state_dict / named_parameters() order): */
typedef struct {
    const float *fc1_w, *fc1_b; /* [H][d_in], [H] */
    const float *fc2_w, *fc2_b; /* [A][H], [A] */
} MlgFFParams;

/* Packed block (floats): w1d [H][Dip], w1o [H][Dob], w1a [A][H] (iff obs_last_action), w1n [N][H] (iff obs_agent_id),
 * b1 [H], w2 [Ap][H], b2 [Ap]: the paddings and transposes of the DRQN block (Dip / Dob / Ap = d_in / d_obs / A rounded
 * up to 16, zero padded) without the GRU blocks and the split-bf16 images. -1 (mlg_last_error()) on bad dims. */
int64_t mlg_ff_packed_size(const MlgAgentDims *d);
int mlg_ff_pack(const MlgAgentDims *d, const MlgFFParams *p, float *packed, void *stream);

/* DQNAgentNetwork.forward over R rows: q [R][A] from inputs [R][d_in]. */
int mlg_ff_forward(const MlgAgentDims *d, const float *packed, const float *inputs, float *q, int32_t R, void *stream);
/* BasicMAC.forward(ep_batch, t) with a feed-forward agent: inputs built from the batch at t as mlg_mac_forward builds
 * them (obs, onehot(a_{t-1}), agent id); batch->rows honoured. */
int mlg_ff_mac_forward(const MlgAgentDims *d, const float *packed, const MlgBatch *batch, int32_t t,
                       float *q /*[B][N][A]*/, void *stream);

/* Backward of mlg_ff_forward (autograd of torch.ops.maleague.dqn_forward), the contract of mlg_agent_backward: it
 * recomputes its forward from `inputs`, writes row activations and deltas to `workspace`
 * (mlg_ff_backward_workspace_floats(dims, R) floats, 16-byte aligned, any contents) and reduces dparams (fc1.weight,
 * fc1.bias, fc2.weight, fc2.bias) in a fixed order without float atomics. dparams is overwritten; R == 0 zeroes it.
 * gq [R][A] NULL = zero upstream gradient, d_inputs [R][d_in] NULL = not wanted. `packed` must be the mlg_ff_pack()
 * block of `p`, 16-byte aligned. */
int64_t mlg_ff_backward_workspace_floats(const MlgAgentDims *d, int32_t R);
int mlg_ff_backward(const MlgAgentDims *d, const MlgFFParams *p, const float *packed, const float *inputs,
                    const float *gq, float *d_inputs, float *dparams, float *workspace, int32_t R, void *stream);

/* One full ParallelStepper.run with a feed-forward agent: mlg_rollout's arguments, run semantics, ring / full-write
 * modes, slot_extent and MlgRunInfo, on the generic fp32 rollout kernel's structure with no hidden state carried
 * across steps; `packed` is the mlg_ff_pack() block. One launch. */
int mlg_rollout_ff(const MlgEnvSpec *spec, MlgEnvState *st, const MlgAgentDims *dims, const float *packed,
                   MlgBatch *batch, MlgRunInfo *info, float epsilon, int32_t test_mode, void *stream);
/* Host only, launches nothing (the contract of mlg_rollout_describe). Names: "ff-lds/tpwK" / "ff-global/tpwK" (the
 * weights w1o, w1a, w1n, b1, w2, b2 in LDS beside the env state / read from global memory, K = 1..4 agent tiles per
 * wave). mlg_rollout_ff takes its decision from the same function. Nonzero (mlg_last_error) where it would refuse the
 * spec or the dims. */
int mlg_rollout_ff_describe(const MlgEnvSpec *spec, const MlgAgentDims *dims, char *name, int32_t name_cap,
                            int64_t *lds_bytes);

/* Packs P flat feed-forward parameter rows (DQNAgentNetwork.PARAM_ORDER: fc1.weight, fc1.bias, fc2.weight, fc2.bias;
 * row p at flat + p * row_stride floats) into packed_pool [P][mlg_ff_packed_size(dims)]; each row equals mlg_ff_pack()
 * of the same parameters bit for bit (the contract of mlg_pack_agent_pool). One launch. NULL pointers, P < 1 and a
 * row_stride below the parameter count are refused through mlg_last_error. */
int mlg_ff_pack_pool(const MlgAgentDims *dims, const float *flat, int64_t row_stride, int32_t P, float *packed_pool,
                     void *stream);

/* One full SelfPlayParallelStepper.run with two feed-forward MACs, in one launch: mlg_rollout_selfplay's arguments and
 * run semantics (`dims` describe one side; home_packed / away_packed are mlg_ff_pack() blocks, 16-byte aligned; the RNG
 * key mlg_env_key(seed, b), the global agent index s * nh + ln as the epsilon stream index, one epsilon per side,
 * reward[0] / reward[1] and ret_away, the ring, full-write and slot_extent modes and the run summary).
 * Structure (mlg_rollout_ff's): a workgroup owns 16 envs for the whole episode, env state in LDS; the agent phase is
 * fc1 -> ReLU -> fc2 per action tile -> masked first-index argmax -> epsilon-greedy redraw, no hidden state carried.
 * The two-side tile layout is mlg_rollout_selfplay_policy's: tps = ceil(16 nh / 16) = nh tiles per side, tile >= tps
 * is the away side, row r = (tile - side * tps) * 16 + col is env r / nh, side-local agent ln = r % nh (the agent-id
 * input); the weight view, the batch and the epsilon of a tile are its side's.
 * Dispatch: tiles = 2 * nh, waves W = min(tiles, 8), tpw = ceil(tiles / W). Names "ffsp-lds/tpwK": both sides' weight
 * images in LDS beside the env state, the home image first; "ffsp-global/tpwK": weights read from global memory (the
 * images do not fit, or MLG_ROLLOUT_GLOBAL_WEIGHTS is set). The two arms differ in where a weight is read from, not in
 * the order of any sum. No float atomics: two runs from the same state are bit-identical.
 * Refused through mlg_last_error, without launching: more than 16 agents per side (the message names the tile count),
 * dims that are not one side of the env, a spec without two policy teams, H outside 32 / 64 / 128. */
int mlg_rollout_selfplay_ff(const MlgEnvSpec *spec, MlgEnvState *st, const MlgAgentDims *dims,
                            const float *home_packed, const float *away_packed, MlgBatch *home, MlgBatch *away,
                            MlgRunInfo *info, float eps_home, float eps_away, int32_t test_mode, void *stream);
/* Host only, launches nothing (the contract of mlg_rollout_describe). mlg_rollout_selfplay_ff takes its decision from
 * the same function. Nonzero (mlg_last_error) where it would refuse the spec or the dims. */
int mlg_rollout_selfplay_ff_describe(const MlgEnvSpec *spec, const MlgAgentDims *dims, char *name, int32_t name_cap,
                                     int64_t *lds_bytes);

/* mlg_crossplay_rollout for feed-forward policies: the same MlgCrossplay block, host checks, per-env outputs and
 * fixed-order summary reduce; packed_pool rows are mlg_ff_packed_size(dims) floats (mlg_ff_pack_pool writes them). Env
 * (pair k, episode e) is bit-identical to env e of one test-mode mlg_rollout_selfplay_ff of that pair under
 * specs[pair.spec] with episode counter episode0. MLG_CROSSPLAY_OBS_WORKSPACE=1 forces the obs / avail rows into
 * `workspace`. No float atomics. */
int64_t mlg_crossplay_ff_workspace_floats(const MlgAgentDims *dims, int32_t n_pairs, int32_t E);
int mlg_crossplay_rollout_ff(const MlgAgentDims *dims, const MlgCrossplay *c, void *stream);

/* ---- Distinct per-agent networks (mac: distinct): agent slot i acts with network i, no parameter sharing --------
 * DistinctMAC (src/marl/controllers/distinct_agents_controller.py). packed_pool [N][mlg_packed_agent_size(dims)]:
 * row i is the mlg_pack_agent() block of network i (mlg_pack_agent_pool writes exactly this); N = dims->n_agents is
 * the pool's row count; 16-byte aligned. dims->obs_agent_id must be 0 (the reference refuses agent ids for distinct
 * networks). A 16-row MFMA tile is one agent across 16 batch rows / envs, its weight view selected by the tile's
 * agent. No float atomics: the same inputs give the same bits. */

/* DistinctMAC.forward(ep_batch, t): the contract of mlg_mac_forward (inputs built from the batch at t as
 * [obs_t | onehot(a_{t-1})], batch->rows honoured, h_in NULL = zeros), q [B][N][A], h_in / h_out [B][N][H]. fc1 is
 * summed in mlg_agent_forward's order over the concatenated row (the dense block), so row (b, i) has the bits of
 * mlg_agent_forward with network i's block on that row: the MAC's differentiable path (maleague::drqn_forward per
 * network) and this call agree bit for bit. */
int mlg_mac_forward_distinct(const MlgAgentDims *dims, const float *packed_pool, const MlgBatch *batch, int32_t t,
                             const float *h_in, float *q, float *h_out, void *stream);

/* One full ParallelStepper.run with a DistinctMAC: mlg_rollout's arguments, run semantics, ring / full-write modes,
 * slot_extent and MlgRunInfo and the counter RNG (the agent index is the epsilon stream index), on the generic fp32
 * rollout kernel's structure with an agent-major agent phase: tile a = agent a of the workgroup's 16 envs, wave w owns
 * tiles w, w + 8, ...; at most 4 tiles per wave, so more than 32 agents are refused (mlg_last_error names the tile
 * count). Weights are read from global memory. A row's arithmetic is the generic kernel's (the column-gather fc1):
 * with N equal networks a run stores the bits of mlg_rollout's generic fp32 kernel. One launch. */
int mlg_rollout_distinct(const MlgEnvSpec *spec, MlgEnvState *st, const MlgAgentDims *dims, const float *packed_pool,
                         MlgBatch *batch, MlgRunInfo *info, float epsilon, int32_t test_mode, void *stream);
/* Host only, launches nothing (the contract of mlg_rollout_describe). Names: "dx-global/tpwK", K = 1..4 agent tiles
 * per wave. mlg_rollout_distinct takes its decision from the same function. Nonzero (mlg_last_error) where it would
 * refuse the spec or the dims. */
int mlg_rollout_distinct_describe(const MlgEnvSpec *spec, const MlgAgentDims *dims, char *name, int32_t name_cap,
                                  int64_t *lds_bytes);

/* One full self-play run with one DRQN per agent slot on both sides (two DistinctMACs), in one launch. It is
 * mlg_rollout_selfplay on the generic fp32 arm with one change: agent ln of side s acts with block ln of side s's
 * pool. home_pool / away_pool: [nh][mlg_packed_agent_size(dims)], the layout mlg_pack_agent_pool writes, 16-byte
 * aligned. `dims` describe one side's MAC: n_agents = nh = spec->n_agents / 2, obs_agent_id must be 0. Everything else
 * is mlg_rollout_selfplay's, bit for bit: the RNG key mlg_env_key(seed, b), the global agent index s * nh + ln as the
 * epsilon stream index, one epsilon per side, reward[0] / reward[1] and ret_away, the ring, full-write and slot_extent
 * modes and the run summary. With nh equal networks per side a run stores the bits of mlg_rollout_selfplay's generic
 * fp32 kernel (MLG_ROLLOUT_KERNEL=v1).
 * Structure (rollout_distinct_kernel's): a workgroup owns 16 envs, env state in LDS, hidden state in VGPRs; the agent
 * phase is agent-major: there are 2 * nh tiles, tile a = s * nh + ln is agent ln of side s across the workgroup's 16
 * envs; wave w owns tiles w, w + W, ... (a wave's tiles may belong to different sides; the side, its batch, its pool
 * and its epsilon are per tile and wave-uniform). Weights are read from global memory. No float atomics: two runs from
 * the same state are bit-identical.
 * Dispatch: tiles = 2 * nh, waves W = min(tiles, 8), tpw = ceil(tiles / W); names "dxsp-global/tpwK": nh 1..4 tpw1,
 * 5..8 tpw2, 9..12 tpw3, 13..16 tpw4. nh > 16, obs_agent_id = 1, H outside 32 / 64 / 128 and dims that do not match
 * the spec are refused through mlg_last_error, without launching. */
int mlg_rollout_selfplay_distinct(const MlgEnvSpec *spec, MlgEnvState *st, const MlgAgentDims *dims,
                                  const float *home_pool, const float *away_pool, MlgBatch *home, MlgBatch *away,
                                  MlgRunInfo *info, float eps_home, float eps_away, int32_t test_mode, void *stream);
/* Host only, launches nothing (the contract of mlg_rollout_describe). mlg_rollout_selfplay_distinct takes its decision
 * from the same function. Nonzero (mlg_last_error) where it would refuse the spec or the dims. */
int mlg_rollout_selfplay_distinct_describe(const MlgEnvSpec *spec, const MlgAgentDims *dims, char *name,
                                           int32_t name_cap, int64_t *lds_bytes);

/* mlg_crossplay_rollout for distinct policies: the same MlgCrossplay block, checks, outputs and summary. packed_pool
 * holds n_pool * nh blocks (nh = dims->n_agents), policy p being blocks [p * nh, (p + 1) * nh); n_pool counts
 * policies. dims->obs_agent_id must be 0; at most 16 agents per side. The tile layout is agent-major as in
 * mlg_rollout_selfplay_distinct; the obs / avail rows, in LDS or in the workspace slice, are read by column = env. Env
 * (pair k, episode e) is bit-identical to env e of one test-mode mlg_rollout_selfplay_distinct of that pair with
 * episode counter episode0. The workspace need is mlg_crossplay_workspace_floats'. */
int mlg_crossplay_rollout_distinct(const MlgAgentDims *dims, const MlgCrossplay *c, void *stream);

/* ---- Prioritized episode replay (replay.hip) ----------------------------------------------------
 * The reference's Memory / BinarySumTree (src/marl/components/replay_buffers/prioritized_replay_buffer.py:8-135) on a
 * flat fp32 priority vector, one entry per replay slot, in slot order. priority = (|err| + e)^a, formed in double and
 * rounded once; priorities must be > 0 (e > 0 makes them so). One launch of one workgroup each; nothing is copied to
 * the host and nothing waits. Every sum and maximum is taken in a fixed order (no float atomics).
 *
 * mlg_per_sample: B stratified draws over the slots [0, n_live). cum[j] = the fp64 inclusive sum of priorities[0..j];
 * total = cum[n_live - 1]; u_i = mlg_u01(mlg_rng(seed, mlg_ctr(draw, 0, MLG_PURPOSE_PER = 6, i)));
 * s_i = (i + u_i) * total / B in fp64; rows[i] = the first slot j with cum[j] >= s_i (BinarySumTree._retrieve in slot
 * order; duplicates are possible); is_weight[i] = (n_live p / total)^-beta over the maximum of the B draws, in fp64,
 * stored as fp32. The scan stays in LDS up to mlg_per_lds_slots() live slots; above that it lives in scan_workspace
 * (n_live doubles, 16-byte aligned, any contents). Refused by name: n_live > mlg_per_max_slots() (>= 65536), B > 4096,
 * a missing or short workspace. */
int32_t mlg_per_lds_slots(void);
int32_t mlg_per_max_slots(void);
int mlg_per_sample(const float *priorities, int32_t n_live, int32_t B, uint64_t seed, uint32_t draw, double beta,
                   int32_t *rows, float *is_weight, double *scan_workspace, int64_t scan_workspace_doubles,
                   void *stream);
/* The priorities of the `count` <= ring_size slots (slot0 + k) % ring_size a rollout or an insert just wrote:
 * *max_priority (a device scalar the caller starts at 1), or with errors [count] the priority of errors[k]; the maximum
 * is raised to the largest priority written. */
int mlg_per_insert(float *priorities, int32_t ring_size, int32_t slot0, int32_t count, const float *errors, double e,
                   double a, float *max_priority, void *stream);
/* After a train call: priorities[rows[b]] = the priority of td_abs[b] (MlgLearnerBufs.td_abs), rows NULL = identity;
 * the maximum is raised. Duplicated slots are the same episode and receive the same value. A row outside
 * [0, n_slots) writes nothing. */
int mlg_per_update(float *priorities, int32_t n_slots, const int32_t *rows, const float *td_abs, int32_t B, double e,
                   double a, float *max_priority, void *stream);

const char *mlg_last_error(void);
const char *mlg_version(void);

#ifdef __cplusplus
}
#endif
#endif
