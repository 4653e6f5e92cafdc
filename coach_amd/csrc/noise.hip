// Device-generated standard normals for the agents' noise_source = "device" mode (TD3's target-policy smoothing noise,
// SAC's three per-update normal arrays, the acting noise of both): Philox4x32-10 (philox.hpp) + one Box-Muller pair per
// call, written with correctly rounded IEEE operations only (+ - * / sqrt, exact conversions, exponent / mantissa bit
// manipulation) in a fixed order — no libm / ocml, no FMA (compiled with -ffp-contract=off) — so that the numpy twin
// tests/noise_ref.py reproduces every bit.
//
//   key     = (seed, rank)
//   counter = (pair index, stream id, event index low word, event index high word ^ kNoiseTag)
// The tag keeps these counters apart from the synthetic environment's (episode, step, block, stream in {0, 1}) under
// its (seed, env id) keys, even when seed and env id equal this generator's seed and rank: a high word of tag or
// tag ^ 1 would need an event index beyond 5.6e18.
//   u1 = (m1 + 1) 2^-53 in (0, 1], u2 = m2 2^-53 in [0, 1)  (m1 = x[31:5] y[31:6], m2 = z[31:5] w[31:6]: 53 bits each)
//   r  = sqrt(-2 ln u1),  z0 = r cos 2 pi u2,  z1 = r sin 2 pi u2
// ln: exponent extraction + 2 atanh((m - 1) / (m + 1)) as its Taylor series on a mantissa m in [sqrt 1/2, sqrt 2);
// cos / sin: the turn u2 is split exactly (integer arithmetic on m2) into a quadrant k and a reduced turn f in
// [-1/2, 1/2) quarter turns, then the Taylor polynomials of sin(pi/2 f) and cos(pi/2 f).  Coefficients are the
// correctly rounded Taylor coefficients, nothing fitted.
#include "rlx_common.hpp"
#include "philox.hpp"

namespace {

constexpr uint32_t kNoiseTag = 0x4E4F4953u;          // "NOIS"
constexpr int kNoiseStreams = 5;                     // of rlx_normal_fill: 0 TD3 smoothing, 1-3 SAC draws 0-2, 4 acting;
                                                     // 5 and up: the NoisyNet layers (noisy_sample_kernel)

constexpr double kTwoM53 = 1.1102230246251565e-16;   // 2^-53
constexpr double kTwoM51 = 4.440892098500626e-16;    // 2^-51
constexpr double kSqrt2 = 1.4142135623730951;
constexpr double kLn2Hi = 0.6931471803691238;        // 0x1.62e42feep-1 (20 trailing zero bits: e * kLn2Hi is exact)
constexpr double kLn2Lo = 1.9082149292705877e-10;    // ln 2 - kLn2Hi

// ln u for u in [2^-53, 1]
__device__ __forceinline__ double ln_unit(double u) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(u);
    int e = (int)((b >> 52) & 0x7FFull) - 1023;
    double m = __longlong_as_double((long long)((b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull));
    if (m >= kSqrt2) {
        m = m * 0.5;
        e += 1;
    }
    const double s = (m - 1.0) / (m + 1.0);          // |s| <= 0.1716
    const double s2 = s * s;
    double p = 0.043478260869565216;                 // 1/23
    p = p * s2 + 0.047619047619047616;               // 1/21
    p = p * s2 + 0.05263157894736842;                // 1/19
    p = p * s2 + 0.058823529411764705;               // 1/17
    p = p * s2 + 0.06666666666666667;                // 1/15
    p = p * s2 + 0.07692307692307693;                // 1/13
    p = p * s2 + 0.09090909090909091;                // 1/11
    p = p * s2 + 0.1111111111111111;                 // 1/9
    p = p * s2 + 0.14285714285714285;                // 1/7
    p = p * s2 + 0.2;                                // 1/5
    p = p * s2 + 0.3333333333333333;                 // 1/3
    p = p * s2 + 1.0;
    const double lm = (s + s) * p;                   // ln m = 2 atanh s
    const double de = (double)e;
    return de * kLn2Hi + (lm + de * kLn2Lo);
}

// sin(pi/2 f), cos(pi/2 f) for f in [-1/2, 1/2]
__device__ __forceinline__ double sin_quarter(double f) {
    const double f2 = f * f;
    double p = 6.0669357311061955e-12;
    p = p * f2 + -6.688035109811468e-10;
    p = p * f2 + 5.692172921967927e-08;
    p = p * f2 + -3.598843235212085e-06;
    p = p * f2 + 0.00016044118478735983;
    p = p * f2 + -0.004681754135318688;
    p = p * f2 + 0.07969262624616705;
    p = p * f2 + -0.6459640975062463;
    p = p * f2 + 1.5707963267948966;
    return f * p;
}

__device__ __forceinline__ double cos_quarter(double f) {
    const double f2 = f * f;
    double p = -5.294400200734623e-13;
    p = p * f2 + 6.565963114979473e-11;
    p = p * f2 + -6.386603083791852e-09;
    p = p * f2 + 4.710874778818172e-07;
    p = p * f2 + -2.5202042373060607e-05;
    p = p * f2 + 0.0009192602748394266;
    p = p * f2 + -0.02086348076335296;
    p = p * f2 + 0.25366950790104803;
    p = p * f2 + -1.2337005501361697;
    return p * f2 + 1.0;
}

__device__ __forceinline__ void box_muller(const rlx::U4 w, double &z0, double &z1) {
    const unsigned long long m1 = ((unsigned long long)(w.x >> 5) << 26) | (w.y >> 6);
    const unsigned long long m2 = ((unsigned long long)(w.z >> 5) << 26) | (w.w >> 6);
    const double u1 = (double)(m1 + 1ull) * kTwoM53;
    const double r = __builtin_sqrt(-2.0 * ln_unit(u1));   // llvm.sqrt.f64: correctly rounded
    // 2 pi u2 = pi/2 (k + f): k the nearest quarter turn, f the rest — exact in integers
    const unsigned long long k = (m2 + (1ull << 50)) >> 51;
    const double f = (double)((long long)m2 - (long long)(k << 51)) * kTwoM51;
    const double s = sin_quarter(f), c = cos_quarter(f);
    double cz, sz;
    switch ((int)(k & 3ull)) {
        case 0: cz = c; sz = s; break;
        case 1: cz = -s; sz = c; break;
        case 2: cz = -c; sz = -s; break;
        default: cz = s; sz = -c; break;
    }
    z0 = r * cz;
    z1 = r * sz;
}

// One thread per Philox call (= one pair of outputs) of every (event, stream); out[event][stream][n].
__global__ void normal_fill_kernel(double *__restrict__ out, const long long *__restrict__ events, int n_events,
                                   int stream0, int n_streams, int n, uint32_t seed, uint32_t rank, double scale) {
    const unsigned pairs = ((unsigned)n + 1u) >> 1;
    const unsigned total = (unsigned)n_events * (unsigned)n_streams * pairs;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned p = i % pairs, es = i / pairs;            // es = event * n_streams + stream
        const unsigned s = es % (unsigned)n_streams, ev_i = es / (unsigned)n_streams;
        const unsigned long long ev = (unsigned long long)events[ev_i];
        const rlx::U4 w = rlx::philox4x32_10(p, (uint32_t)stream0 + s, (uint32_t)ev, (uint32_t)(ev >> 32) ^ kNoiseTag,
                                             seed, rank);
        double z0, z1;
        box_muller(w, z0, z1);
        double *o = out + (size_t)es * (size_t)n + 2 * (size_t)p;
        o[0] = z0 * scale;
        if (2 * p + 1 < (unsigned)n) o[1] = z1 * scale;
    }
}

// The factorised NoisyNet layers' noise (csrc/noisy_dense.hip): f(e) = sign(e) sqrt(|e|) of standard normals e, in fp64
// (sqrt is correctly rounded), then rounded once to fp32.  One workgroup per layer; layer L's vectors of pass P are
// streams kNoiseStreams + 3 (RLX_NOISY_PASSES L + P) + {0: f_in, 1: f_out, 2: f_b} at the event index held in
// counters[RLX_NOISY_PASSES L + P], which the workgroup reads from device memory and then advances by one: a
// replayed graph draws fresh values.
constexpr int kMaxNoisyLayers = RLX_NOISY_MAX_LAYERS;
struct NoisySample {
    rlx_noisy_layer l[kMaxNoisyLayers];
};

__device__ __forceinline__ double signed_sqrt(double v) {
    const double s = __builtin_sqrt(__builtin_fabs(v));
    return v < 0.0 ? -s : s;
}

__global__ void __launch_bounds__(256) noisy_sample_kernel(const NoisySample s, long long *__restrict__ counters,
                                                           int pass, uint32_t seed, uint32_t rank) {
    const rlx_noisy_layer &L = s.l[blockIdx.x];
    long long *cnt = counters + (size_t)L.layer * RLX_NOISY_PASSES + pass;
    const unsigned long long ev = (unsigned long long)*cnt;
    const uint32_t stream0 = (uint32_t)kNoiseStreams + 3u * (uint32_t)(RLX_NOISY_PASSES * L.layer + pass);
    const unsigned pin = ((unsigned)L.K + 1u) >> 1, pn = ((unsigned)L.N + 1u) >> 1;
    for (unsigned i = threadIdx.x; i < pin + 2u * pn; i += blockDim.x) {
        const unsigned which = i < pin ? 0u : (i < pin + pn ? 1u : 2u);
        const unsigned p = which == 0u ? i : (which == 1u ? i - pin : i - pin - pn);
        const unsigned n = which == 0u ? (unsigned)L.K : (unsigned)L.N;
        const size_t base = which == 0u ? 0 : (which == 1u ? (size_t)L.K : (size_t)L.K + (size_t)L.N);
        const rlx::U4 w = rlx::philox4x32_10(p, stream0 + which, (uint32_t)ev, (uint32_t)(ev >> 32) ^ kNoiseTag, seed,
                                             rank);
        double z0, z1;
        box_muller(w, z0, z1);
        const double f0 = signed_sqrt(z0), f1 = signed_sqrt(z1);
        const size_t o = base + 2 * (size_t)p;
        L.f[o] = (float)f0;
        if (L.f64) L.f64[o] = f0;
        if (2 * p + 1 < n) {
            L.f[o + 1] = (float)f1;
            if (L.f64) L.f64[o + 1] = f1;
        }
    }
    __syncthreads();                      // every thread has read the counter
    if (threadIdx.x == 0) *cnt = (long long)(ev + 1ull);
}

}  // namespace

extern "C" {

int rlx_noisy_sample(const rlx_noisy_layer *layers_host, int n_layers, long long *counters, int pass,
                     unsigned int seed, unsigned int rank, void *stream) {
    RLX_REQUIRE(layers_host && counters, "rlx_noisy_sample: null pointer");
    RLX_REQUIRE(n_layers >= 1 && n_layers <= kMaxNoisyLayers, "rlx_noisy_sample: need 1..%d layers (got %d)",
                kMaxNoisyLayers, n_layers);
    RLX_REQUIRE(pass >= 0 && pass < RLX_NOISY_PASSES, "rlx_noisy_sample: bad pass %d (0..%d)", pass,
                RLX_NOISY_PASSES - 1);
    NoisySample s;
    for (int i = 0; i < n_layers; ++i) {
        const rlx_noisy_layer &l = layers_host[i];
        RLX_REQUIRE(l.f, "rlx_noisy_sample: null pointer in layer %d", i);
        RLX_REQUIRE(l.K > 0 && l.N > 0 && l.layer >= 0 && l.layer < (1 << 20),
                    "rlx_noisy_sample: bad shape in layer %d (K=%d N=%d index=%d)", i, l.K, l.N, l.layer);
        for (int j = 0; j < i; ++j)
            RLX_REQUIRE(layers_host[j].layer != l.layer, "rlx_noisy_sample: layer index %d given twice", l.layer);
        s.l[i] = l;
    }
    RLX_LAUNCH((noisy_sample_kernel), n_layers, 256, 0, rlx::as_stream(stream), s, counters, pass, (uint32_t)seed,
               (uint32_t)rank);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

int rlx_normal_fill(double *out, const long long *events, int n_events, int stream0, int n_streams, int n,
                    unsigned int seed, unsigned int rank, double scale, void *stream) {
    RLX_REQUIRE(out && events, "rlx_normal_fill: null pointer");
    RLX_REQUIRE(n > 0 && n_events > 0, "rlx_normal_fill: bad sizes (n = %d, n_events = %d)", n, n_events);
    RLX_REQUIRE(stream0 >= 0 && n_streams > 0 && (long long)stream0 + n_streams <= kNoiseStreams,
                "rlx_normal_fill: bad stream range (stream0 = %d, n_streams = %d; streams 0..%d)", stream0, n_streams,
                kNoiseStreams - 1);
    const long long total = (long long)n_events * n_streams * ((n + 1LL) / 2);
    RLX_REQUIRE(total <= 0x7FFFFFFFLL, "rlx_normal_fill: too many values (%lld pairs)", total);
    RLX_LAUNCH((normal_fill_kernel), rlx::grid_for(total, 256), 256, 0, rlx::as_stream(stream), out, events,
               n_events, stream0, n_streams, n, (uint32_t)seed, (uint32_t)rank, scale);
    RLX_LAUNCH_CHECK();
    return RLX_OK;
}

}  // extern "C"
