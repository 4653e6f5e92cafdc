// Batch RL from a logged dataset — the device half of EpisodicExperienceReplay.load_csv
// (rl_coach/memories/episodic/episodic_experience_replay.py:440-495) on gfx950.
//
// The reference builds one Python Transition per file row (DataFrame.iterrows) and sends every episode through the
// input filter.  Here the host parses the file once into flat tables (coach_amd/memories/episodic/csv_dataset.py),
// uploads them once, and ONE launch turns them into replay rows: transition t reads file row src[t] (state, action,
// reward, probabilities) and file row src_next[t] (next state) and writes the memory's own columns at row
// first_row + t.  Features and rewards are rounded to fp32 once (round-to-nearest-even, numpy's astype); the fp32
// reward then goes through the reward filters' arithmetic (reward_filter.hpp, the function rlx_reward_filter runs), so a
// loaded reward carries the bits the acting path would have stored.  Compiled with -ffp-contract=off like filters.hip.
//
// One 64-lane wave per transition, four transitions per workgroup, lanes stride the features: a gather-and-convert
// launch bound by memory latency.  Bit-exact numpy twin: tests/dataset_ref.py.
#include "rlx_common.hpp"
#include "reward_filter.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for NaN

__global__ void __launch_bounds__(kWave * kWavesPerBlock)
dataset_ingest_kernel(const double *__restrict__ features, long long ld_f, const int *__restrict__ actions,
                      const double *__restrict__ rewards, const float *__restrict__ probs, long long ld_p,
                      long long n_rows, int D, int A, const int *__restrict__ src, const int *__restrict__ src_next,
                      const unsigned char *__restrict__ last, long long n_transitions, int is_episodic,
                      long long first_row, double rescale, int use_hi, double hi, int use_lo, double lo,
                      float *__restrict__ mem_obs, float *__restrict__ mem_next_obs, int *__restrict__ mem_action,
                      float *__restrict__ mem_reward, unsigned char *__restrict__ mem_game_over,
                      float *__restrict__ mem_probs, int *__restrict__ status) {
    const int lane = threadIdx.x & (kWave - 1);
    const long long wave = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const long long waves = (long long)gridDim.x * kWavesPerBlock;
    for (long long t = wave; t < n_transitions; t += waves) {
        const long long s = src[t], sn = src_next[t];
        const bool s_ok = s >= 0 && s < n_rows, sn_ok = sn >= 0 && sn < n_rows;
        const long long row = first_row + t;
        int bits = (s_ok && sn_ok) ? 0 : 4;
        // an index outside the tables reads nothing: its cells are written as zeros
        const double *f = features + (s_ok ? s : 0) * ld_f, *fn = features + (sn_ok ? sn : 0) * ld_f;
        for (int j = lane; j < D; j += kWave) {
            const float a = s_ok ? (float)f[j] : 0.f, b = sn_ok ? (float)fn[j] : 0.f;
            if (!finite_f32(a) || !finite_f32(b)) bits |= 2;
            mem_obs[row * D + j] = a;
            mem_next_obs[row * D + j] = b;
        }
        if (mem_probs) {
            const float *p = probs + (s_ok ? s : 0) * ld_p;
            for (int j = lane; j < A; j += kWave) mem_probs[row * A + j] = s_ok ? p[j] : 0.f;
        }
        if (lane == 0) {
            int a = s_ok ? actions[s] : 0;
            if (a < 0 || a >= A) {
                bits |= 1;
                a = 0;
            }
            const float r = s_ok ? (float)rewards[s] : 0.f;
            if (!finite_f32(r)) bits |= 2;
            mem_action[row] = a;
            mem_reward[row] = rlx::reward_filter_value(r, rescale, use_hi, hi, use_lo, lo);
            mem_game_over[row] = (last[t] != 0 && is_episodic) ? 1 : 0;
        }
        if (bits) atomicOr(status, bits);
    }
}

}  // namespace

extern "C" {

int rlx_dataset_ingest(const double *features, long long ld_features, const int *actions, const double *rewards,
                       const float *probabilities, long long ld_probabilities, long long n_rows, int D, int A,
                       const int *src, const int *src_next, const unsigned char *last, long long n_transitions,
                       int is_episodic, long long first_row, long long mem_rows, double rescale_factor, int has_clip,
                       double clipping_low, double clipping_high, float *mem_obs, float *mem_next_obs, int *mem_action,
                       float *mem_reward, unsigned char *mem_game_over, float *mem_probabilities, int *status,
                       void *stream) {
    RLX_REQUIRE(features && actions && rewards && src && src_next && last && mem_obs && mem_next_obs && mem_action &&
                    mem_reward && mem_game_over && status,
                "rlx_dataset_ingest: null pointer");
    RLX_REQUIRE((probabilities == nullptr) == (mem_probabilities == nullptr),
                "rlx_dataset_ingest: the probabilities table and the memory's column come together");
    RLX_REQUIRE(D >= 1 && D <= 4096, "rlx_dataset_ingest: 1 <= D <= 4096 features (got %d)", D);
    RLX_REQUIRE(A >= 1 && A <= 18, "rlx_dataset_ingest: 1 <= A <= 18 actions (got %d)", A);
    RLX_REQUIRE(n_transitions >= 1, "rlx_dataset_ingest: no transitions (N=%lld)", n_transitions);
    RLX_REQUIRE(n_rows >= 1 && n_rows <= 2147483647LL, "rlx_dataset_ingest: 1 <= file rows < 2^31 (got %lld)", n_rows);
    RLX_REQUIRE(first_row >= 0 && n_transitions <= mem_rows && first_row <= mem_rows - n_transitions,
                "rlx_dataset_ingest: rows %lld .. %lld are outside the memory's %lld rows", first_row,
                first_row + n_transitions - 1, mem_rows);
    RLX_REQUIRE(ld_features >= D, "rlx_dataset_ingest: leading dimension %lld of the features is below D=%d",
                ld_features, D);
    RLX_REQUIRE(!probabilities || ld_probabilities >= A,
                "rlx_dataset_ingest: leading dimension %lld of the probabilities is below A=%d", ld_probabilities, A);
    RLX_REQUIRE(rescale_factor != 0.0, "The reward rescale value can not be set to 0");
    RLX_REQUIRE(!has_clip || clipping_low <= clipping_high,
                "The reward clipping low must be lower than the reward clipping max");
    // `if self.clipping_high:` / `if self.clipping_low:` — a bound equal to 0 is not applied (as rlx_reward_filter)
    const int use_hi = has_clip && clipping_high != 0.0;
    const int use_lo = has_clip && clipping_low != 0.0;
    const int grid = rlx::grid_for(n_transitions, kWavesPerBlock);
    RLX_LAUNCH((dataset_ingest_kernel), grid, kWave * kWavesPerBlock, 0, rlx::as_stream(stream), features, ld_features,
               actions, rewards, probabilities, ld_probabilities, n_rows, D, A, src, src_next, last, n_transitions,
               is_episodic, first_row, rescale_factor, use_hi, clipping_high, use_lo, clipping_low, mem_obs,
               mem_next_obs, mem_action, mem_reward, mem_game_over, mem_probabilities, status);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
