// BitFlip for N environments per GPU — the toy problem behind the reference's BitFlip_DQN / BitFlip_DQN_HER presets
// (rl_coach/environments/toy_problems/bit_flip.py:54-90, created by GymVectorEnvironment(level='...bit_flip:BitFlip')).
//
//     step(a):   state[a] = !state[a];  steps += 1
//     reward     0 when state == goal, else -1
//     done       state == goal or steps >= max_steps
//     mean_zero  emitted values are (x - 0.5) / 0.5, i.e. -1 / +1 instead of 0 / 1
//
// The observation is ONE fp32 vector of 2 L values, [desired_goal | state] (the reference's embedders concatenate in
// sorted() name order); `bits` keeps the same layout as bytes: bits[e][0..L) the goal, bits[e][L..2L) the state.
//
// Reset draws: the reference calls Python's random.choice per bit; here they come from the counter-based Philox stream
// the other device environments use: key (seed, env id), counter (episode, word index, 0, kStreamBitFlip); a draw word
// is the FIRST output word of that call, one bit per state / goal bit, low bit first, nw = ceil(L / 32) words per
// vector.  Words [0, nw) are the state, words [nw (1 + t), nw (2 + t)) the t-th goal draw; the goal is redrawn
// (t = 1 .. 32) while it equals the state, and after 32 redraws bit 0 of the goal is flipped instead, so the loop is
// finite by construction.  A pure function of (seed, env, episode): tests/bit_flip_ref.py restates it in numpy.
// One thread per env, O(L) bytes each: latency-bound plumbing like cartpole.hip, not a roofline kernel.
#include "rlx_common.hpp"
#include "philox.hpp"

namespace {

constexpr uint32_t kStreamBitFlip = 3;
constexpr int kMaxGoalRedraws = 32;

__device__ __forceinline__ uint32_t draw_word(uint32_t seed, uint32_t env, uint32_t ep, uint32_t w) {
    return rlx::philox4x32_10(ep, w, 0u, kStreamBitFlip, seed, env).x;
}

// the first goal and state of episode `ep` into b[0 .. 2L)
__device__ void draw_episode(uint32_t seed, uint32_t env, uint32_t ep, int L, unsigned char *b) {
    const int nw = (L + 31) / 32;
    for (int w = 0; w < nw; ++w) {
        const uint32_t x = draw_word(seed, env, ep, (uint32_t)w);
        for (int i = 32 * w; i < L && i < 32 * w + 32; ++i) b[L + i] = (x >> (i & 31)) & 1u;
    }
    for (int t = 0; t <= kMaxGoalRedraws; ++t) {
        bool equal = true;
        for (int w = 0; w < nw; ++w) {
            const uint32_t x = draw_word(seed, env, ep, (uint32_t)(nw * (1 + t) + w));
            for (int i = 32 * w; i < L && i < 32 * w + 32; ++i) {
                const unsigned char g = (x >> (i & 31)) & 1u;
                b[i] = g;
                equal = equal && g == b[L + i];
            }
        }
        if (!equal) return;
    }
    b[0] ^= 1;
}

__device__ __forceinline__ float emit(unsigned char bit, int mean_zero) {
    return bit ? 1.0f : (mean_zero ? -1.0f : 0.0f);
}

__global__ void bitflip_reset_kernel(unsigned char *bits, float *obs, int *episode, int *steps, int n_env, int L,
                                     int mean_zero, uint32_t seed, uint32_t env_id0, int next_episode) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    const int ep = next_episode ? episode[e] + 1 : 0;       // a forced reset mid-episode starts the NEXT episode's draw
    unsigned char *b = bits + (size_t)e * 2 * L;
    draw_episode(seed, env_id0 + e, (uint32_t)ep, L, b);
    for (int i = 0; i < 2 * L; ++i) obs[(size_t)e * 2 * L + i] = emit(b[i], mean_zero);
    episode[e] = ep;
    steps[e] = 0;
}

__global__ void bitflip_step_kernel(const int *__restrict__ action, unsigned char *bits, int *episode, int *steps,
                                    float *next_obs, float *reset_obs, float *reward, unsigned char *done, int n_env,
                                    int L, int max_steps, int mean_zero, uint32_t seed, uint32_t env_id0, int *status) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    unsigned char *b = bits + (size_t)e * 2 * L;
    const int a = action[e];
    if (a < 0 || a >= L) atomicOr(status, 2);                // outside Discrete(L): nothing is flipped, nothing indexed
    else b[L + a] ^= 1;
    const int t = steps[e] + 1;
    bool equal = true;
    for (int i = 0; i < L; ++i) equal = equal && b[i] == b[L + i];
    for (int i = 0; i < 2 * L; ++i) next_obs[(size_t)e * 2 * L + i] = emit(b[i], mean_zero);
    reward[e] = equal ? 0.0f : -1.0f;
    const bool is_done = equal || t >= max_steps;
    done[e] = is_done ? 1 : 0;
    if (is_done) {
        const int ep = episode[e] + 1;
        draw_episode(seed, env_id0 + e, (uint32_t)ep, L, b);
        for (int i = 0; i < 2 * L; ++i) reset_obs[(size_t)e * 2 * L + i] = emit(b[i], mean_zero);
        episode[e] = ep;
        steps[e] = 0;
    } else {
        steps[e] = t;
    }
}

}  // namespace

extern "C" {

int rlx_bitflip_reset(unsigned char *bits, float *obs, int *episode, int *steps, int n_env, int bit_length,
                      int mean_zero, unsigned int seed, unsigned int env_id0, int next_episode, void *stream) {
    RLX_REQUIRE(bits && obs && episode && steps, "rlx_bitflip_reset: null pointer");
    RLX_REQUIRE(n_env > 0 && bit_length > 0, "rlx_bitflip_reset: bad sizes (n_env %d, bit_length %d)", n_env,
                bit_length);
    RLX_LAUNCH((bitflip_reset_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), bits, obs, episode, steps,
               n_env, bit_length, mean_zero, seed, env_id0, next_episode);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_bitflip_step(const int *action, unsigned char *bits, int *episode, int *steps, float *next_obs,
                     float *reset_obs, float *reward, unsigned char *game_over, int n_env, int bit_length,
                     int max_steps, int mean_zero, unsigned int seed, unsigned int env_id0, int *status,
                     void *stream) {
    RLX_REQUIRE(action && bits && episode && steps && next_obs && reset_obs && reward && game_over && status,
                "rlx_bitflip_step: null pointer");
    RLX_REQUIRE(n_env > 0 && bit_length > 0 && max_steps > 0,
                "rlx_bitflip_step: bad sizes (n_env %d, bit_length %d, max_steps %d)", n_env, bit_length, max_steps);
    RLX_LAUNCH((bitflip_step_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), action, bits, episode, steps,
               next_obs, reset_obs, reward, game_over, n_env, bit_length, max_steps, mean_zero, seed, env_id0, status);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
