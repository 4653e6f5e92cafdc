// ExplorationChain for N environments per GPU — the toy problem behind the reference's ExplorationChain_* presets
// (rl_coach/environments/toy_problems/exploration_chain.py:24-94, created by a 'module:Class' level).
//
//     step(0):   state -= 1 unless state == 0            step(1):   state += 1 unless state == chain_length - 1
//     reward     left_state_reward at state 0, right_state_reward at state chain_length - 1, else 0 (after the move)
//     done       steps >= max_steps
//
// The observation is one fp32 vector of chain_length values: Therm sets ones at [0, state], OneHot at state alone.
// There is nothing random: every episode starts at start_state and lasts exactly max_steps steps, so the host knows which
// envs finished without reading game_over back.  An action other than 0 / 1 (the reference raises) sets status bit 1 and
// moves nothing; the step still counts.  tests/exploration_chain_ref.py restates both kernels in numpy.
// One thread per env, O(chain_length) words each: latency-bound plumbing like bit_flip.hip, not a roofline kernel.
#include "rlx_common.hpp"

namespace {

__device__ __forceinline__ void emit(float *obs, int L, int state, int therm) {
    for (int i = 0; i < L; ++i) obs[i] = (therm ? i <= state : i == state) ? 1.0f : 0.0f;
}

__global__ void chain_reset_kernel(int *state, int *steps, float *obs, int n_env, int L, int start_state, int therm) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    state[e] = start_state;
    steps[e] = 0;
    emit(obs + (size_t)e * L, L, start_state, therm);
}

__global__ void chain_step_kernel(const int *__restrict__ action, int *state, int *steps, float *next_obs,
                                  float *reset_obs, float *reward, unsigned char *done, int n_env, int L,
                                  int start_state, int max_steps, int therm, float left_reward, float right_reward,
                                  int *status) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    const int a = action[e];
    int s = state[e];
    s = s < 0 ? 0 : (s >= L ? L - 1 : s);                    // (stays inside the observation whatever the word holds)
    if (a == 0) s -= s > 0 ? 1 : 0;
    else if (a == 1) s += s < L - 1 ? 1 : 0;
    else atomicOr(status, 2);                                // outside Discrete(2): nothing moves
    const int t = steps[e] + 1;
    emit(next_obs + (size_t)e * L, L, s, therm);
    reward[e] = s == 0 ? left_reward : (s == L - 1 ? right_reward : 0.0f);
    const bool is_done = t >= max_steps;
    done[e] = is_done ? 1 : 0;
    if (is_done) {
        emit(reset_obs + (size_t)e * L, L, start_state, therm);
        state[e] = start_state;
        steps[e] = 0;
    } else {
        state[e] = s;
        steps[e] = t;
    }
}

}  // namespace

extern "C" {

int rlx_chain_reset(int *state, int *steps, float *obs, int n_env, int chain_length, int start_state, int therm,
                    void *stream) {
    RLX_REQUIRE(state && steps && obs, "rlx_chain_reset: null pointer");
    RLX_REQUIRE(n_env > 0 && chain_length > 3 && start_state >= 0 && start_state < chain_length,
                "rlx_chain_reset: bad sizes (n_env %d, chain_length %d > 3, start_state %d)", n_env, chain_length,
                start_state);
    RLX_LAUNCH((chain_reset_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), state, steps, obs, n_env,
               chain_length, start_state, therm);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_chain_step(const int *action, int *state, int *steps, float *next_obs, float *reset_obs, float *reward,
                   unsigned char *game_over, int n_env, int chain_length, int start_state, int max_steps, int therm,
                   float left_state_reward, float right_state_reward, int *status, void *stream) {
    RLX_REQUIRE(action && state && steps && next_obs && reset_obs && reward && game_over && status,
                "rlx_chain_step: null pointer");
    RLX_REQUIRE(n_env > 0 && chain_length > 3 && start_state >= 0 && start_state < chain_length && max_steps > 0,
                "rlx_chain_step: bad sizes (n_env %d, chain_length %d > 3, start_state %d, max_steps %d)", n_env,
                chain_length, start_state, max_steps);
    RLX_LAUNCH((chain_step_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), action, state, steps, next_obs,
               reset_obs, reward, game_over, n_env, chain_length, start_state, max_steps, therm, left_state_reward,
               right_state_reward, status);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
