// Hindsight Experience Replay: the relabelled copies of ONE finished episode, written on the device
// (rl_coach/memories/episodic/episodic_hindsight_experience_replay.py:108-145 `store_episode`).
//
// The episode's T real transitions lie time-major in the replay ring: step t at row
//     r(t) = ((first_step + t) mod ring_steps) * n_env + env               (r < R = n_env * ring_steps).
// Every payload column has (1 + k) * R rows; copy j (0 <= j < k) of real row r lives at row R + r * k + j.
// For base transition t < n_base (n_base = T, or T - 1 under Future) and copy j the host drew the step offset
// sel[t * k + j] of the SELECTED transition (np.random.choice, in the reference's walk order); the copy is
//     obs / next_obs       row r(t) with the desired-goal slice [goal_at, goal_at + goal_dim) replaced by the goal,
//                          goal = obs[r(sel)][achieved_at .. achieved_at + goal_dim): the selected transition's STATE
//     action               row r(t), action_row_bytes bytes (int32, or action_dim floats)
//     reward, game_over    ReachingGoal: distance(goal, next_obs[r(t)][achieved slice]) <= threshold ?
//                          (goal_reaching_reward, 1) : (default_reward, 0)
// The distance is fp64, summed in index order (no contraction): Euclidean sqrt(sum d^2) or Manhattan sum |d|;
// tests/her_ref.py is the numpy restatement.  One 64-lane workgroup per copy: lanes stride the row, lane 0 sums the
// distance — a few hundred bytes per copy, launched once per finished episode.
#include "rlx_common.hpp"

namespace {

struct HerArgs {
    float *obs, *next_obs;
    unsigned char *action;
    float *reward;
    unsigned char *game_over;
    const int *sel;
    long long first_step, ring_steps;
    int length, n_base, k, env, n_env;
    int obs_dim, goal_at, achieved_at, goal_dim, action_row_bytes, metric;
    double threshold;
    float reach_reward, default_reward;
    int *status;
};

__global__ void her_relabel_kernel(HerArgs a) {
    const int copy = blockIdx.x;                 // t * k + j
    if (copy >= a.n_base * a.k) return;
    const int t = copy / a.k, j = copy - t * a.k;
    const int st = a.sel[copy];
    if (st < 0 || st >= a.length) {              // never indexes with it
        if (threadIdx.x == 0) atomicOr(a.status, 4);
        return;
    }
    const long long R = (long long)a.n_env * a.ring_steps;
    const long long r = ((a.first_step + t) % a.ring_steps) * a.n_env + a.env;
    const long long rs = ((a.first_step + st) % a.ring_steps) * a.n_env + a.env;
    const long long d = R + r * a.k + j;
    const float *goal = a.obs + rs * a.obs_dim + a.achieved_at;
    const float *src_o = a.obs + r * a.obs_dim, *src_n = a.next_obs + r * a.obs_dim;
    float *dst_o = a.obs + d * a.obs_dim, *dst_n = a.next_obs + d * a.obs_dim;
    for (int i = threadIdx.x; i < a.obs_dim; i += blockDim.x) {
        const int g = i - a.goal_at;
        const bool in_goal = g >= 0 && g < a.goal_dim;
        dst_o[i] = in_goal ? goal[g] : src_o[i];
        dst_n[i] = in_goal ? goal[g] : src_n[i];
    }
    const unsigned char *src_a = a.action + r * a.action_row_bytes;
    unsigned char *dst_a = a.action + d * a.action_row_bytes;
    for (int i = threadIdx.x; i < a.action_row_bytes; i += blockDim.x) dst_a[i] = src_a[i];
    if (threadIdx.x == 0) {
        const float *ach = src_n + a.achieved_at;
        double sum = 0.0;
        for (int i = 0; i < a.goal_dim; ++i) {
            const double diff = (double)goal[i] - (double)ach[i];
            sum = sum + (a.metric == RLX_HER_EUCLIDEAN ? diff * diff : fabs(diff));
        }
        const double dist = a.metric == RLX_HER_EUCLIDEAN ? sqrt(sum) : sum;
        const bool reached = dist <= a.threshold;
        a.reward[d] = reached ? a.reach_reward : a.default_reward;
        a.game_over[d] = reached ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int rlx_her_relabel_episode(float *obs, float *next_obs, void *action, float *reward, unsigned char *game_over,
                            const int *selected_steps, long long first_step, int length, int n_base, int k, int env,
                            int n_env, long long ring_steps, int obs_dim, int goal_at, int achieved_at, int goal_dim,
                            int action_row_bytes, int metric, double threshold, float goal_reaching_reward,
                            float default_reward, int *status, void *stream) {
    RLX_REQUIRE(obs && next_obs && action && reward && game_over && selected_steps && status,
                "rlx_her_relabel_episode: null pointer");
    RLX_REQUIRE(n_env > 0 && env >= 0 && env < n_env && ring_steps > 0 && first_step >= 0,
                "rlx_her_relabel_episode: bad ring (env %d of %d, ring_steps %lld, first_step %lld)", env, n_env,
                ring_steps, first_step);
    RLX_REQUIRE(length > 0 && length <= ring_steps && n_base > 0 && n_base <= length && k > 0,
                "rlx_her_relabel_episode: bad episode (length %d, n_base %d, k %d, ring_steps %lld)", length, n_base, k,
                ring_steps);
    RLX_REQUIRE((long long)n_env * ring_steps * (1 + (long long)k) < (1ll << 40),
                "rlx_her_relabel_episode: the extended ring is too large");
    RLX_REQUIRE(obs_dim > 0 && goal_dim > 0 && goal_at >= 0 && goal_at + goal_dim <= obs_dim && achieved_at >= 0 &&
                    achieved_at + goal_dim <= obs_dim && action_row_bytes > 0,
                "rlx_her_relabel_episode: bad slices (obs_dim %d, goal [%d, +%d), achieved at %d, action bytes %d)",
                obs_dim, goal_at, goal_dim, achieved_at, action_row_bytes);
    RLX_REQUIRE(metric == RLX_HER_EUCLIDEAN || metric == RLX_HER_MANHATTAN,
                "rlx_her_relabel_episode: metric must be RLX_HER_EUCLIDEAN or RLX_HER_MANHATTAN (got %d)", metric);
    HerArgs a{obs, next_obs, (unsigned char *)action, reward, game_over, selected_steps, first_step, ring_steps,
              length, n_base, k, env, n_env, obs_dim, goal_at, achieved_at, goal_dim, action_row_bytes, metric,
              threshold, goal_reaching_reward, default_reward, status};
    RLX_LAUNCH((her_relabel_kernel), n_base * k, 64, 0, rlx::as_stream(stream), a);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
