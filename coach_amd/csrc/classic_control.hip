// Pendulum-v0 and Acrobot-v1 for N environments per GPU — the two classic-control levels of gym 0.12.5
// (gym/envs/classic_control/pendulum.py, acrobot.py; `GymVectorEnvironment(level='Pendulum-v0' | 'Acrobot-v1')`, the
// level of rl_coach/presets/Acrobot_DDQN_BCQ_BatchRL.py:97) whose physics are fp64 arithmetic plus sin / cos, like
// CartPole's (cartpole.hip), behind gym's TimeLimit (200 and 500 steps).  Shaped like rlx_cartpole_*: fp64 state per env,
// one thread per env with the whole state in registers, no LDS, one launch per vector step, auto-reset where an episode
// ends, reset states from the Philox stream under CartPole's scheme (key = (seed, env id), counter = (episode, word
// pair, 0, kStreamReset), 53-bit uniforms like numpy's random_sample, mapped in fp64 as numpy's uniform(low, high) does:
// low + (high - low) * u).  gym is not installable here; the CPU restatement is in tests/test_classic_control.py.
// sin / cos go through rlx::libm_sin_full / libm_cos_full (libm_sincos_full.hpp: glibc's algorithm with its range
// reduction, |x| < 2^20), and the file is compiled without contraction: every operation below rounds once, in numpy's
// evaluation order.
//
// Pendulum (state th, thdot; action fp32 [n_env][1]) — where each rounding happens:
//     u      = clip(a, -2, 2)                       in fp32 (exact), then widened to fp64 (exact)
//     an     = fmod(th + pi, 2 pi) [+ 2 pi if negative] - pi     Python's floored modulo: one rounding in th + pi, fmod is
//              exact, one rounding where 2 pi is added back, one in - pi
//     cost   = (an * an + 0.1 * (thdot * thdot)) + 0.001 * (u * u)              six roundings, left to right
//     thdot' = thdot + ((-15.0 * sin(th + pi)) + 3.0 * u) * 0.05     -3 g / (2 l) = -15 and 3 / (m l^2) = 3 are exact
//     th'    = th + thdot' * 0.05                   with the UNCLIPPED thdot', as gym does; then thdot' = clip(thdot', -8, 8)
//     reward = (float)(-cost);  obs = (float)(cos th', sin th', thdot')
// Acrobot (state theta1, theta2, dtheta1, dtheta2; action int32 in {0, 1, 2}, torque a - 1, "book" dynamics, no torque
// noise): one RK4 step of dt = 0.2 — k1 = f(y), k2 = f(y + 0.1 k1), k3 = f(y + 0.1 k2), k4 = f(y + 0.2 k3),
// y' = y + (0.2 / 6.0) * (((k1 + 2 k2) + 2 k3) + k4) per component (the torque component's derivative is 0, so it stays a)
// — with f = gym's _dsdt, its constants folded exactly as Python folds them (m1 = m2 = l1 = I1 = I2 = 1, lc1 = lc2 = 0.5,
// g = 9.8; multiplications by 1, 2 and 0.5 are exact, so folding them changes no bit; x ** 2 is x * x).  Then both angles
// are wrapped into [-pi, pi] by gym's subtract / add loop, dtheta1 bound to +-4 pi, dtheta2 to +-9 pi; terminal when
// -cos theta1 - cos(theta2 + theta1) > 1; reward 0 on the terminal step, else -1.
//
// status: bit 0 = an argument outside libm_*_full's range (or an angle the wrap loop cannot bring home in 64 turns: gym
// would loop on); bit 1 = an Acrobot action outside {0, 1, 2} or a non-finite Pendulum action — that env does not move
// on that step (next state = state, reward 0), the step counts.
// ~25 sin / cos evaluations and ~250 flops per Acrobot env-step, 3 and ~30 per Pendulum env-step: latency-bound plumbing.
#include "rlx_common.hpp"
#include "philox.hpp"
#include "libm_sincos_full.hpp"

namespace {

constexpr uint32_t kStreamReset = 2;
constexpr double kPi = 3.141592653589793;

__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {        // numpy random_sample: (a >> 5, b >> 6)
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

// ---------------------------------------------------------------- Pendulum
__device__ __forceinline__ void pendulum_reset_state(uint32_t seed, uint32_t env, uint32_t ep, double (&s)[2]) {
    const rlx::U4 r0 = rlx::philox4x32_10(ep, 0u, 0u, kStreamReset, seed, env);
    s[0] = -kPi + (kPi - -kPi) * u53(r0.x, r0.y);           // uniform(low=-high, high=high), high = (pi, 1)
    s[1] = -1.0 + (1.0 - -1.0) * u53(r0.z, r0.w);
}
__device__ __forceinline__ void pendulum_obs(const double (&s)[2], float *o, int *dom) {
    o[0] = (float)rlx::libm_cos_full(s[0], dom);
    o[1] = (float)rlx::libm_sin_full(s[0], dom);
    o[2] = (float)s[1];
}

__global__ void pendulum_reset_kernel(double *state, float *obs, int *episode, int *steps, int n_env, uint32_t seed,
                                      uint32_t env_id0, int next_episode) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    const int ep = next_episode ? episode[e] + 1 : 0;       // a forced reset mid-episode starts the NEXT episode's draw
    double s[2];
    pendulum_reset_state(seed, env_id0 + e, (uint32_t)ep, s);
    int dom = 0;                                            // |th| <= pi: never out of range
    pendulum_obs(s, obs + 3 * (size_t)e, &dom);
    state[2 * (size_t)e] = s[0];
    state[2 * (size_t)e + 1] = s[1];
    episode[e] = ep;
    steps[e] = 0;
}

__global__ void pendulum_step_kernel(const float *__restrict__ action, double *state, int *episode, int *steps,
                                     float *next_obs, float *reset_obs, double *next_state64, float *reward,
                                     unsigned char *done, int n_env, int max_episode_steps, uint32_t seed,
                                     uint32_t env_id0, int *status) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    const double th = state[2 * (size_t)e], thdot = state[2 * (size_t)e + 1];
    const float a = action[e];
    const bool bad = !isfinite(a);
    int dom = 0;
    double ns[2] = {th, thdot};
    float r = 0.0f;
    if (!bad) {
        const double u = (double)fminf(fmaxf(a, -2.0f), 2.0f);
        double m = fmod(th + kPi, 2 * kPi);                 // Python's a % b for b > 0
        if (m < 0.0) m = m + 2 * kPi;
        const double an = m - kPi;
        const double cost = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u);
        double newthdot = thdot + (-15.0 * rlx::libm_sin_full(th + kPi, &dom) + 3.0 * u) * 0.05;
        ns[0] = th + newthdot * 0.05;
        ns[1] = newthdot < -8.0 ? -8.0 : (newthdot > 8.0 ? 8.0 : newthdot);
        r = (float)(-cost);
    }
    pendulum_obs(ns, next_obs + 3 * (size_t)e, &dom);
    if (next_state64) {
        next_state64[2 * (size_t)e] = ns[0];
        next_state64[2 * (size_t)e + 1] = ns[1];
    }
    if (bad || dom) atomicOr(status, (bad ? 2 : 0) | (dom ? 1 : 0));
    const int t = steps[e] + 1;
    const bool is_done = t >= max_episode_steps;            // TimeLimit only: the pendulum never terminates
    reward[e] = r;
    done[e] = is_done ? 1 : 0;
    if (is_done) {
        const int ep = episode[e] + 1;
        pendulum_reset_state(seed, env_id0 + e, (uint32_t)ep, ns);
        pendulum_obs(ns, reset_obs + 3 * (size_t)e, &dom);
        episode[e] = ep;
        steps[e] = 0;
    } else {
        steps[e] = t;
    }
    state[2 * (size_t)e] = ns[0];
    state[2 * (size_t)e + 1] = ns[1];
}

// ---------------------------------------------------------------- Acrobot
__device__ __forceinline__ void acrobot_reset_state(uint32_t seed, uint32_t env, uint32_t ep, double (&s)[4]) {
    const rlx::U4 r0 = rlx::philox4x32_10(ep, 0u, 0u, kStreamReset, seed, env);
    const rlx::U4 r1 = rlx::philox4x32_10(ep, 1u, 0u, kStreamReset, seed, env);
    s[0] = -0.1 + (0.1 - -0.1) * u53(r0.x, r0.y);           // uniform(low=-0.1, high=0.1, size=(4,))
    s[1] = -0.1 + (0.1 - -0.1) * u53(r0.z, r0.w);
    s[2] = -0.1 + (0.1 - -0.1) * u53(r1.x, r1.y);
    s[3] = -0.1 + (0.1 - -0.1) * u53(r1.z, r1.w);
}
// writes the six observations, returns cos(theta1) for the terminal test
__device__ __forceinline__ double acrobot_obs(const double (&s)[4], float *o, int *dom) {
    const double c1 = rlx::libm_cos_full(s[0], dom);
    o[0] = (float)c1;
    o[1] = (float)rlx::libm_sin_full(s[0], dom);
    o[2] = (float)rlx::libm_cos_full(s[1], dom);
    o[3] = (float)rlx::libm_sin_full(s[1], dom);
    o[4] = (float)s[2];
    o[5] = (float)s[3];
    return c1;
}

// gym's _dsdt, "book" dynamics: y = (theta1, theta2, dtheta1, dtheta2), torque a -> (dtheta1, dtheta2, ddtheta1, ddtheta2)
__device__ __forceinline__ void acrobot_dsdt(const double (&y)[4], double a, double (&k)[4], int *dom) {
    const double theta1 = y[0], theta2 = y[1], dtheta1 = y[2], dtheta2 = y[3];
    const double g = 9.8;
    const double c2 = rlx::libm_cos_full(theta2, dom), s2 = rlx::libm_sin_full(theta2, dom);
    // d1 = m1 lc1^2 + m2 (l1^2 + lc2^2 + 2 l1 lc2 cos theta2) + I1 + I2;  d2 = m2 (lc2^2 + l1 lc2 cos theta2) + I2
    const double d1 = 0.25 + (1.0 + 0.25 + c2) + 1.0 + 1.0;
    const double d2 = (0.25 + 0.5 * c2) + 1.0;
    // phi2 = m2 lc2 g cos(theta1 + theta2 - pi/2):  (1 * 0.5 * 9.8) is 4.9
    const double phi2 = (0.5 * g) * rlx::libm_cos_full(theta1 + theta2 - kPi / 2.0, dom);
    // phi1 = -m2 l1 lc2 dtheta2^2 sin theta2 - 2 m2 l1 lc2 dtheta2 dtheta1 sin theta2 + (m1 lc1 + m2 l1) g cos(theta1 - pi/2) + phi2
    const double phi1 = -0.5 * (dtheta2 * dtheta2) * s2 - dtheta2 * dtheta1 * s2 +
                        (1.5 * g) * rlx::libm_cos_full(theta1 - kPi / 2.0, dom) + phi2;
    // ddtheta2 = (a + d2 / d1 phi1 - m2 l1 lc2 dtheta1^2 sin theta2 - phi2) / (m2 lc2^2 + I2 - d2^2 / d1)
    const double ddtheta2 = (a + d2 / d1 * phi1 - 0.5 * (dtheta1 * dtheta1) * s2 - phi2) / (1.25 - d2 * d2 / d1);
    const double ddtheta1 = -(d2 * ddtheta2 + phi1) / d1;
    k[0] = dtheta1;
    k[1] = dtheta2;
    k[2] = ddtheta1;
    k[3] = ddtheta2;
}
// gym's wrap(x, -pi, pi).  The 64 turns (both loops together) only guard against hanging on a huge or infinite angle:
// a bounded velocity moves an angle by at most 9 pi * 0.2 per step, one turn, so the count is reached from a hand-written
// state alone, and the result departs from gym's only for |x| beyond about 128 pi — flagged in status bit 0.
__device__ __forceinline__ double acrobot_wrap(double x, int *dom) {
    const double diff = kPi - -kPi;
    int turns = 0;
    while (x > kPi && turns < 64) { x = x - diff; ++turns; }
    while (x < -kPi && turns < 64) { x = x + diff; ++turns; }
    if (turns == 64) *dom = 1;
    return x;
}
__device__ __forceinline__ double acrobot_bound(double x, double m, double M) {      // min(max(x, m), M) as Python orders it
    const double lo = m > x ? m : x;
    return M < lo ? M : lo;
}

__global__ void acrobot_reset_kernel(double *state, float *obs, int *episode, int *steps, int n_env, uint32_t seed,
                                     uint32_t env_id0, int next_episode) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    const int ep = next_episode ? episode[e] + 1 : 0;
    double s[4];
    acrobot_reset_state(seed, env_id0 + e, (uint32_t)ep, s);
    int dom = 0;
    acrobot_obs(s, obs + 6 * (size_t)e, &dom);
#pragma unroll
    for (int j = 0; j < 4; ++j) state[4 * (size_t)e + j] = s[j];
    episode[e] = ep;
    steps[e] = 0;
}

__global__ void acrobot_step_kernel(const int *__restrict__ action, double *state, int *episode, int *steps,
                                    float *next_obs, float *reset_obs, double *next_state64, float *reward,
                                    unsigned char *done, int n_env, int max_episode_steps, uint32_t seed,
                                    uint32_t env_id0, int *status) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_env) return;
    double y0[4], ns[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ns[j] = y0[j] = state[4 * (size_t)e + j];
    const int act = action[e];
    const bool bad = act < 0 || act > 2;
    int dom = 0;
    if (!bad) {
        const double a = (double)(act - 1);                 // AVAIL_TORQUE = [-1., 0., +1]
        const double dt = 0.2, dt2 = dt / 2.0;
        double k1[4], k2[4], k3[4], k4[4], y[4];
        acrobot_dsdt(y0, a, k1, &dom);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = y0[j] + dt2 * k1[j];
        acrobot_dsdt(y, a, k2, &dom);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = y0[j] + dt2 * k2[j];
        acrobot_dsdt(y, a, k3, &dom);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = y0[j] + dt * k3[j];
        acrobot_dsdt(y, a, k4, &dom);
#pragma unroll
        for (int j = 0; j < 4; ++j) ns[j] = y0[j] + dt / 6.0 * (k1[j] + 2 * k2[j] + 2 * k3[j] + k4[j]);
        ns[0] = acrobot_wrap(ns[0], &dom);
        ns[1] = acrobot_wrap(ns[1], &dom);
        ns[2] = acrobot_bound(ns[2], -(4 * kPi), 4 * kPi);
        ns[3] = acrobot_bound(ns[3], -(9 * kPi), 9 * kPi);
    }
    const double c1 = acrobot_obs(ns, next_obs + 6 * (size_t)e, &dom);
    const bool terminal = -c1 - rlx::libm_cos_full(ns[1] + ns[0], &dom) > 1.0;
    if (next_state64) {
#pragma unroll
        for (int j = 0; j < 4; ++j) next_state64[4 * (size_t)e + j] = ns[j];
    }
    if (bad || dom) atomicOr(status, (bad ? 2 : 0) | (dom ? 1 : 0));
    const int t = steps[e] + 1;
    const bool is_done = terminal || t >= max_episode_steps;
    reward[e] = (terminal || bad) ? 0.0f : -1.0f;
    done[e] = is_done ? 1 : 0;
    if (is_done) {
        const int ep = episode[e] + 1;
        acrobot_reset_state(seed, env_id0 + e, (uint32_t)ep, ns);
        acrobot_obs(ns, reset_obs + 6 * (size_t)e, &dom);
        episode[e] = ep;
        steps[e] = 0;
    } else {
        steps[e] = t;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) state[4 * (size_t)e + j] = ns[j];
}

__global__ void libm_sincos_full_kernel(const double *x, double *s, double *c, int n, int *status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int dom = 0;
    s[i] = rlx::libm_sin_full(x[i], &dom);
    c[i] = rlx::libm_cos_full(x[i], &dom);
    if (dom) atomicOr(status, 1);
}

}  // namespace

extern "C" {

int rlx_pendulum_reset(double *state, float *obs, int *episode, int *steps, int n_env, unsigned int seed,
                       unsigned int env_id0, int next_episode, void *stream) {
    RLX_REQUIRE(state && obs && episode && steps, "rlx_pendulum_reset: null pointer");
    RLX_REQUIRE(n_env > 0, "rlx_pendulum_reset: n_env must be positive (got %d)", n_env);
    RLX_LAUNCH((pendulum_reset_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), state, obs, episode, steps,
               n_env, seed, env_id0, next_episode);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_pendulum_step(const float *action, double *state, int *episode, int *steps, float *next_obs, float *reset_obs,
                      double *next_state64, float *reward, unsigned char *game_over, int n_env,
                      int max_episode_steps, unsigned int seed, unsigned int env_id0, int *status, void *stream) {
    RLX_REQUIRE(action && state && episode && steps && next_obs && reset_obs && reward && game_over && status,
                "rlx_pendulum_step: null pointer");
    RLX_REQUIRE(n_env > 0 && max_episode_steps > 0, "rlx_pendulum_step: bad sizes (n_env %d, max_episode_steps %d)",
                n_env, max_episode_steps);
    RLX_LAUNCH((pendulum_step_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), action, state, episode, steps,
               next_obs, reset_obs, next_state64, reward, game_over, n_env, max_episode_steps, seed, env_id0, status);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_acrobot_reset(double *state, float *obs, int *episode, int *steps, int n_env, unsigned int seed,
                      unsigned int env_id0, int next_episode, void *stream) {
    RLX_REQUIRE(state && obs && episode && steps, "rlx_acrobot_reset: null pointer");
    RLX_REQUIRE(n_env > 0, "rlx_acrobot_reset: n_env must be positive (got %d)", n_env);
    RLX_LAUNCH((acrobot_reset_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), state, obs, episode, steps,
               n_env, seed, env_id0, next_episode);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_acrobot_step(const int *action, double *state, int *episode, int *steps, float *next_obs, float *reset_obs,
                     double *next_state64, float *reward, unsigned char *game_over, int n_env, int max_episode_steps,
                     unsigned int seed, unsigned int env_id0, int *status, void *stream) {
    RLX_REQUIRE(action && state && episode && steps && next_obs && reset_obs && reward && game_over && status,
                "rlx_acrobot_step: null pointer");
    RLX_REQUIRE(n_env > 0 && max_episode_steps > 0, "rlx_acrobot_step: bad sizes (n_env %d, max_episode_steps %d)",
                n_env, max_episode_steps);
    RLX_LAUNCH((acrobot_step_kernel), (n_env + 63) / 64, 64, 0, rlx::as_stream(stream), action, state, episode, steps,
               next_obs, reset_obs, next_state64, reward, game_over, n_env, max_episode_steps, seed, env_id0, status);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_libm_sincos_full(const double *x, double *sin_out, double *cos_out, int n, int *status, void *stream) {
    RLX_REQUIRE(x && sin_out && cos_out && status && n > 0, "rlx_libm_sincos_full: bad arguments");
    RLX_LAUNCH((libm_sincos_full_kernel), (n + 255) / 256, 256, 0, rlx::as_stream(stream), x, sin_out, cos_out, n,
               status);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
