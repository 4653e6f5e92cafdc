// A finished episode's way into the replay of an n-step agent (Rainbow), ONE launch per episode.
//
// Replaces, in the reference (paths under rl_coach/):
//   * Episode.update_transitions_rewards_and_bootstrap_data    core_types.py:803-820 (every transition's next_state becomes
//                                                               the state n steps ahead — or the episode's last next state —
//                                                               with should_bootstrap_next_state saying which)
//   * Episode.update_discounted_rewards                         core_types.py:771-801 (n_step_discounted_rewards)
//   * Agent.handle_episode_ended's store loop                   agents/agent.py:571-574 (the transitions in episode order)
//
// The source is one env's staged episode: row k (0 <= k < T) of columns laid out [n_env][stage_len].  The destination is
// T consecutive rows of a replay's struct-of-arrays ring starting at dst0, modulo ring_rows.  The n-step return is
// rlx::episode_nstep_return (episode_returns.hpp), the body rlx_episode_nstep_returns runs: bit-identical to it and to the
// reference's column.  Compiled with -ffp-contract=off.
#include "rlx_common.hpp"
#include "episode_returns.hpp"

namespace {

struct NstepStoreArgs {
    const float *s_obs, *s_next_obs;     // [n_env][stage_len][obs_dim]
    const int *s_action;                 // [n_env][stage_len][action_words]
    const float *s_reward;               // [n_env][stage_len]
    const unsigned char *s_game_over;    // [n_env][stage_len]
    int env, stage_len, T, n_step, obs_dim, action_words;
    double discount;
    float *obs, *next_obs;               // [ring_rows][obs_dim]
    int *action;                         // [ring_rows][action_words]
    float *reward;
    unsigned char *game_over;
    double *n_step_returns;
    unsigned char *bootstrap;
    long long dst0, ring_rows;
};

// One workgroup (a wave) per transition k.
__global__ void __launch_bounds__(64) nstep_episode_store_kernel(const NstepStoreArgs a) {
    const int k = blockIdx.x, t = threadIdx.x, T = a.T, D = a.obs_dim;
    const size_t base = (size_t)a.env * a.stage_len;
    const size_t dst = (size_t)((a.dst0 + k) % a.ring_rows);
    const int c = a.n_step < T ? a.n_step : T;
    const bool boot = k + c < T;                                    // core_types.py:811-818
    const float *so = a.s_obs + (base + k) * D;
    const float *sn = boot ? a.s_obs + (base + k + c) * D : a.s_next_obs + (base + T - 1) * D;
    for (int i = t; i < D; i += 64) {
        a.obs[dst * D + i] = so[i];
        a.next_obs[dst * D + i] = sn[i];
    }
    for (int i = t; i < a.action_words; i += 64)
        a.action[dst * a.action_words + i] = a.s_action[(base + k) * a.action_words + i];
    if (t == 0) {
        const float *r = a.s_reward + base;
        a.reward[dst] = r[k];
        a.game_over[dst] = a.s_game_over[base + k];
        a.n_step_returns[dst] = rlx::episode_nstep_return(r, k, T, c, a.discount, [](int j) { return j; });
        a.bootstrap[dst] = boot ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int rlx_nstep_episode_store(const float *staged_obs, const float *staged_next_obs, const int *staged_actions,
                            const float *staged_rewards, const unsigned char *staged_game_overs, int env, int n_env,
                            int stage_len, int length, int n_step, double discount, int obs_dim, int action_words,
                            float *obs, float *next_obs, int *actions, float *rewards, unsigned char *game_overs,
                            double *n_step_discounted_rewards, unsigned char *should_bootstrap_next_state,
                            long long dst0, long long ring_rows, void *stream) {
    RLX_REQUIRE(staged_obs && staged_next_obs && staged_actions && staged_rewards && staged_game_overs && obs &&
                    next_obs && actions && rewards && game_overs && n_step_discounted_rewards &&
                    should_bootstrap_next_state,
                "rlx_nstep_episode_store: null pointer");
    RLX_REQUIRE(n_env > 0 && env >= 0 && env < n_env && length > 0 && length <= stage_len && obs_dim > 0 &&
                    action_words > 0,
                "rlx_nstep_episode_store: bad episode geometry (env=%d of %d, length=%d, staged rows=%d)", env, n_env,
                length, stage_len);
    RLX_REQUIRE(ring_rows > 0 && length <= ring_rows && dst0 >= 0 && dst0 < ring_rows,
                "rlx_nstep_episode_store: the episode (%d transitions from row %lld) does not fit the ring (%lld rows)",
                length, dst0, ring_rows);
    RLX_REQUIRE(n_step >= 1, "n-step should be an integer with value >= 1");
    NstepStoreArgs a;
    a.s_obs = staged_obs; a.s_next_obs = staged_next_obs; a.s_action = staged_actions; a.s_reward = staged_rewards;
    a.s_game_over = staged_game_overs; a.env = env; a.stage_len = stage_len; a.T = length; a.n_step = n_step;
    a.obs_dim = obs_dim; a.action_words = action_words; a.discount = discount; a.obs = obs; a.next_obs = next_obs;
    a.action = actions; a.reward = rewards; a.game_over = game_overs; a.n_step_returns = n_step_discounted_rewards;
    a.bootstrap = should_bootstrap_next_state; a.dst0 = dst0; a.ring_rows = ring_rows;
    RLX_LAUNCH((nstep_episode_store_kernel), length, 64, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
