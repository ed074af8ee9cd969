// mzdriver.hip — device glue of the sampled-MCTS driver loop (include/mzdriver.h).
//
// The reference driver (core/mcts/tree_search/mcts_sampled.py:114-172) moves every simulation's
// network outputs to the host and prepares the next tree inputs with numpy.  These kernels do the
// same arithmetic on the device, one wavefront per root, so that the results equal the numpy
// expressions bit for bit:
//   - np.exp on float32: numpy 2.x's SIMD float32 exponential (AVX512F and AVX2/FMA3 loops; same
//     algorithm): k = rint(x * log2 e); y = x + k*(-ln2_hi) + k*(-ln2_lo) with FMAs; exp(y) = P5(y)
//     / Q2(y), Horner with FMAs; result scaled by 2^k.  Validated here against np.exp on ~2e7
//     float32 inputs including the denormal range (tests/test_driver.py checks it on every host).
//   - np.sum(axis=-1) of a contiguous row of n <= 128 elements: pairwise summation base case, 8
//     interleaved accumulators r[j] += a[i + j], combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
//     then the n % 8 tail; n < 8 sums sequentially from 0.
//   - float16 arrays (policy logits under torch autocast): numpy's half loops evaluate each
//     operation in float32 and round the result to half; half sums accumulate in float32 and
//     round once.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <type_traits>

#include "../../include/mzdriver.h"
#include "mz_internal.h"

namespace {

constexpr int kWave = 64;

// numpy's float32 exp constants (rational minimax approximation on [-ln2/2, ln2/2]).
constexpr float kLog2e = 1.442695040888963387f;
constexpr float kLn2Hi = -6.93145752e-1f;
constexpr float kLn2Lo = -1.42860677e-6f;
constexpr float kP0 = 9.999999999980870924916e-01f;
constexpr float kP1 = 7.257664613233124478488e-01f;
constexpr float kP2 = 2.473615434895520810817e-01f;
constexpr float kP3 = 5.114512081637298353406e-02f;
constexpr float kP4 = 6.757896990527504603057e-03f;
constexpr float kP5 = 5.082762527590693718096e-04f;
constexpr float kQ0 = 1.0f;
constexpr float kQ1 = -2.742335390411667452936e-01f;
constexpr float kQ2 = 2.159509375685829852307e-02f;

__device__ float np_expf(float x) {
    if (x != x) return x + x;                 // NaN
    if (x > 88.72283935546875f) return INFINITY;
    if (x < -104.0f) return 0.0f;             // below half the smallest denormal
    const float k = rintf(x * kLog2e);        // product rounded to f32, then to nearest even
    float y = fmaf(k, kLn2Hi, x);
    y = fmaf(k, kLn2Lo, y);
    float num = fmaf(kP5, y, kP4);
    num = fmaf(num, y, kP3);
    num = fmaf(num, y, kP2);
    num = fmaf(num, y, kP1);
    num = fmaf(num, y, kP0);
    float den = fmaf(kQ2, y, kQ1);
    den = fmaf(den, y, kQ0);
    return ldexpf(num / den, (int)k);
}

__device__ __forceinline__ float to_half_and_back(float v) { return __half2float(__float2half_rn(v)); }

// np.exp of a float16 array.  numpy does not always evaluate it as float32 exp rounded to half: on
// AVX512_SKX hosts its half loop uses a vectorised float32 exponential of its own, which rounds to a
// different half for a few inputs (4 of the 63,488 finite halves on this image's numpy 2.2).  The
// host hands its numpy's answer for every half bit pattern (mz_set_half_exp_table); without that
// table the kernels round numpy's float32 SIMD exp to half.
__device__ __forceinline__ float np_exp_half(float d, const unsigned short *table) {
    if (table) return __half2float(__ushort_as_half(table[__half_as_ushort(__float2half_rn(d))]));
    return to_half_and_back(np_expf(d));
}

template <bool F16>
__device__ __forceinline__ float np_exp_as(float d, const unsigned short *table) {
    if constexpr (F16) return np_exp_half(d, table);
    return np_expf(d);
}

template <bool F16>
__device__ __forceinline__ float round_as(float v) {
    if constexpr (F16) return to_half_and_back(v);
    return v;
}

template <bool F16>
__device__ __forceinline__ float load_elem(const void *p, long long i) {
    if constexpr (F16) return __half2float(static_cast<const __half *>(p)[i]);
    return static_cast<const float *>(p)[i];
}

__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

// numpy's `x ** e` for an array x >= 0 of the logits' dtype and the exponent e = 1 / sampled_tau,
// which NEP 50 casts to that dtype (the caller passes it so rounded).  numpy's exponents 2 and 0.5
// are np.square / np.sqrt, its float16 loop is libm's powf rounded to half, and libm's powf is
// correctly rounded in all but ~0.07 % of inputs: the float64 pow rounded to float is the correctly
// rounded result (up to results within a float64 ulp of a float midpoint), so all of these agree
// with it.  numpy's float32 loop on AVX-512 hosts is SVML's powf, which is not correctly rounded
// (about 1 in 5 results is one ulp off); that case is not reproducible here.
// use_pow: 0 no power (exponent 1.0: numpy returns the array), kPowSquare / kPowSqrt (numpy's
// fast_scalar_power for the Python exponents 2.0 and 0.5), kPowGeneral
constexpr int kPowGeneral = 1, kPowSquare = 2, kPowSqrt = 3;
template <bool F16>
__device__ __forceinline__ float np_pow_as(float x, float e, int mode) {
    if (mode == kPowSquare) return round_as<F16>(x * x);
    if (mode == kPowSqrt) return round_as<F16>(sqrtf(x));  // (IEEE: -fhip-fp32-correctly-rounded-divide-sqrt)
    return round_as<F16>((float)pow((double)x, (double)e));
}

int pow_mode(double inv) {
    return inv == 1.0 ? 0 : inv == 2.0 ? kPowSquare : inv == 0.5 ? kPowSqrt : kPowGeneral;
}

// The softmax of a row whose exponentials sum to a NaN -- the row holds a NaN, or its maximum is
// infinite, so that x - max is inf - inf -- is a NaN in every element, and so is beta.  Which NaN is the
// host's arithmetic, not the GPU's (whose subtraction negates a NaN second operand, sign included):
// x86-64 hands a NaN operand on as it stands (np.nan: the positive quiet NaN) and answers inf - inf with
// its default NaN, the negative one; numpy's float32 exp returns the positive quiet NaN for either,
// its float16 loops keep the sign.  So the element is set by hand: negative only for a float16 row
// without a NaN of its own.
template <bool F16>
__device__ __forceinline__ float np_softmax_nan(bool nan_any) {
    return __uint_as_float((F16 && !nan_any) ? 0xffc00000u : 0x7fc00000u);
}

// float64 -> float16 with one rounding (round to nearest, ties to even), as numpy casts a float64
// result into a float16 array (npy_double_to_half); via float32 it would round twice.
__device__ float round_d2h(double d) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    const unsigned short sign = (unsigned short)((b >> 48) & 0x8000u);
    const int ex = (int)((b >> 52) & 0x7ff);
    const unsigned long long mant = b & 0xfffffffffffffull;
    unsigned short h;
    if (ex == 0x7ff) {
        h = (unsigned short)(sign | 0x7c00u | (mant ? 0x200u : 0u));  // inf / NaN
    } else if (ex == 0) {
        h = sign;  // double zero / subnormal: far below half's range
    } else {
        int e = ex - 1023 + 15;                               // half's biased exponent
        const unsigned long long m = (1ull << 52) | mant;     // 53-bit significand
        const int shift = (e >= 1) ? 42 : 42 + (1 - e);       // bits dropped (subnormal results: more)
        if (shift >= 64) {
            h = sign;
        } else {
            unsigned long long q = m >> shift;
            const unsigned long long rem = m & ((1ull << shift) - 1ull), half = 1ull << (shift - 1);
            if (rem > half || (rem == half && (q & 1ull))) ++q;
            if (e >= 1) {
                if (q == (1ull << 11)) {  // the rounding carried into the next binade
                    q >>= 1;
                    ++e;
                }
                h = (e >= 31) ? (unsigned short)(sign | 0x7c00u) : (unsigned short)(sign | (e << 10) | (q & 0x3ffu));
            } else {
                h = (unsigned short)(sign | q);  // subnormal (q == 0x400: the smallest normal)
            }
        }
    }
    return __half2float(__ushort_as_half(h));
}

// a float64 result stored into an array of the logits' dtype
template <bool F16>
__device__ __forceinline__ float store_d(double v) {
    if constexpr (F16) return round_d2h(v);
    return (float)v;
}

// ------------------------------------------------------------------------------------------------
// One wave per row of A <= 255 actions: lane l holds the actions l + 64 j, j < T = ceil(A / 64), in
// registers (T is a template parameter: the tile loops unroll; T = 1 is one lane per action).  The
// row reductions and row bodies below are stated once for every T.
//
// np.sum(axis=-1) of a row of n > 128 elements is no longer one base case: numpy's pairwise sum
// splits at n2 = n / 2, n2 -= n2 % 8 and adds pairwise(a, n2) + pairwise(a + n2, n - n2),
// recursively.  For n <= 255 the first half (<= 120) is always a base case and the second (<= 135)
// splits at most once more, so a row is at most three base-case blocks, each starting at a multiple
// of 8, joined from the right: s0, s0 + s1 or s0 + (s1 + s2); a row of n <= 128 is the one block
// (0, n).  The launcher walks the recursion once (sum_plan) and hands the kernel the blocks.
constexpr int kWideMax = 255;       // the handle's own limit (a node packs its action in 8 bits)
constexpr int kPairwiseBlock = 128; // numpy's PW_BLOCKSIZE
constexpr int kMaxBlocks = 3;

// the base-case blocks of numpy's pairwise sum over n elements, 1 <= n <= 255, in row order: byte b is
// the length of block b (1..128; 0: no such block), and a block starts where the one before it ends.
// (Past 257 elements a left half would split too, and the join would no longer be the right-nested one.)
unsigned sum_plan(int n) {
    unsigned lens = 0u;
    int shift = 0;
    while (n > kPairwiseBlock) {  // pairwise(a, n2) + pairwise(a + n2, n - n2): n2 <= 120 is a base case
        int n2 = n / 2;
        n2 -= n2 % 8;
        lens |= (unsigned)n2 << shift;
        n -= n2;
        shift += 8;
    }
    return lens | (unsigned)n << shift;
}

// The kernels take the plan in place of A, which it holds: one block (A itself) for one tile, else the
// lengths' sum.
template <int T>
__device__ __forceinline__ int plan_len(unsigned plan) {
    if constexpr (T == 1) return (int)plan;
    return (int)((plan & 0xffu) + (plan >> 8 & 0xffu) + (plan >> 16));
}

// v of another lane of the same row of 16 lanes, by a DPP control (no LDS round trip as __shfl_xor's):
// lane l ^ 1, lane l ^ 2, and lane l ^ 7 (the other quad of l's group of 8)
constexpr int kDppXor1 = 0xb1, kDppXor2 = 0x4e, kDppHalfMirror = 0x141;  // quad_perm [1,0,3,2], [2,3,0,1]
template <int kCtrl>
__device__ __forceinline__ float lane_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xf, 0xf, true));
}

// lane `lane`'s v (a constant lane) in every lane
__device__ __forceinline__ float lane_value(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// np.sum over the row whose element l + 64 j is v[j] (lds[64 T] is the workgroup's; plan = sum_plan(A));
// result in every lane.  Lanes 8 b + i run accumulator i of block b; the 8 accumulators combine as a
// butterfly, which is numpy's ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) in every lane of the group (float
// addition commutes; after two steps a quad's lanes agree, so any lane of the other quad serves the
// third); lane 8 b adds the block's n % 8 tail; the block sums join from the right.  A block of fewer
// than 8 elements (the row itself, A < 8) is numpy's sequential sum from 0.0f: its lanes load no
// accumulator, so the butterfly leaves 0.0f and the tail adds elements 0 .. len - 1 in order.
// With one tile the row is the one block (0, A), which the plan says too: stated in place, the compiler
// sees the block's bounds and keeps the short loop short (measured: profiles/glue_unify/README.md).
// Every lane of the wave is active here: the callers' control flow is workgroup-uniform.
template <int T>
__device__ float np_row_sum(const float (&v)[T], int l, int A, unsigned plan, float *lds) {
#pragma unroll
    for (int j = 0; j < T; ++j)
        if (l + kWave * j < A) lds[l + kWave * j] = v[j];
    __syncthreads();
    const int blk = l >> 3, i = l & 7;
    int start = 0, len = blk == 0 ? A : 0;
    if constexpr (T > 1) {
        const int len0 = (int)(plan & 0xffu), len1 = (int)(plan >> 8 & 0xffu);
        start = blk == 0 ? 0 : blk == 1 ? len0 : len0 + len1;
        len = blk < kMaxBlocks ? (int)(plan >> (8 * blk) & 0xffu) : 0;
    }
    // (lanes past the last block idle with len = 0)
    const int n8 = len - len % 8;
    float r = 0.f;
    if (len >= 8) {  // (the row holds lds[start + i] only for i < len)
        r = lds[start + i];
        for (int k = 8; k < n8; k += 8) r += lds[start + k + i];
    }
    r += lane_dpp<kDppXor1>(r);
    r += lane_dpp<kDppXor2>(r);
    r += lane_dpp<kDppHalfMirror>(r);
    if (i == 0)
        for (int k = n8; k < len; ++k) r += lds[start + k];
    float s = lane_value(r, 0);
    if constexpr (T > 1) {
        const float s1 = lane_value(r, 8), s2 = lane_value(r, 16);
        if (plan >> 16)
            s = s + (s1 + s2);
        else if (plan >> 8)
            s = s + s1;
    }
    __syncthreads();  // (the row is read: the next sum may overwrite it)
    return s;
}

// np.max(axis=-1) of the row: a NaN anywhere makes it that NaN (one ballot per tile; the first in
// action order where the row holds several)
template <int T>
__device__ __forceinline__ float np_row_max(const float (&x)[T], int l, int A) {
    bool nan_any = false;
    float m = -INFINITY, nan_v = 0.f;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const bool on = l + kWave * j < A;
        const unsigned long long nan_mask = __ballot(on && (x[j] != x[j]));
        if (!nan_any && nan_mask) {  // (wave-uniform)
            nan_any = true;
            nan_v = __shfl(x[j], __ffsll((long long)nan_mask) - 1, kWave);
        }
        m = fmaxf(m, on ? x[j] : -INFINITY);
    }
    return nan_any ? nan_v : wave_max(m);
}

// np.argmax of the row of A elements that starts at element `row` of p (mcts_sampled.py:136-145): the
// smallest action holding a NaN if there is one, else the smallest action equal to the maximum; the
// result in every lane.  Action l + 64 j orders by tile first, so the tiles are scanned in order and
// the first set ballot bit taken inside a tile.
template <bool F16, int T>
__device__ __forceinline__ int np_argmax_row(const void *p, long long row, int A, int l) {
    float v[T];
    float m = -INFINITY;
    int idx = -1;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int a = l + kWave * j;
        const bool on = a < A;
        v[j] = on ? load_elem<F16>(p, row + a) : -INFINITY;
        m = fmaxf(m, v[j]);
        const unsigned long long nan_mask = __ballot(on && (v[j] != v[j]));
        if (idx < 0 && nan_mask) idx = kWave * j + __ffsll((long long)nan_mask) - 1;
    }
    if (idx < 0) {  // (wave-uniform)
        m = wave_max(m);
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const unsigned long long hit = __ballot(l + kWave * j < A && v[j] == m);
            if (idx < 0 && hit) idx = kWave * j + __ffsll((long long)hit) - 1;
        }
    }
    return idx;
}

// mcts_sampled.py:158-161 (+ .astype(np.float32), :169-170) for root t, lane l of its wave: the body
// of k_policy_glue and of role 0 of k_policy_glue_later.  The agent's logits start at element col_off
// of the root's row; the A results go to row `out_row` of probs / beta.  A row that holds a NaN, or
// whose maximum is infinite, sums to a NaN and is set by hand (np_softmax_nan), so the GPU's own
// x - max is good enough in front of it.
template <bool F16, int T>
__device__ __forceinline__ void policy_glue_row(const void *logits, long long row_stride, long long col_off, int A,
                                                unsigned plan, int use_pow, float tau_inv, float *probs,
                                                float *beta, const unsigned short *hexp, int t,
                                                long long out_row, int l, float *lds) {
    float x[T], e[T], p[T], q[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int a = l + kWave * j;
        x[j] = a < A ? load_elem<F16>(logits, (long long)t * row_stride + col_off + a) : -INFINITY;
    }
    const float m = np_row_max<T>(x, l, A);
    const bool nan_any = m != m;
#pragma unroll
    for (int j = 0; j < T; ++j) e[j] = np_exp_as<F16>(round_as<F16>(x[j] - m), hexp);
    const float s = round_as<F16>(np_row_sum<T>(e, l, A, plan, lds));
#pragma unroll
    for (int j = 0; j < T; ++j) {
        p[j] = round_as<F16>(e[j] / s);
        // `** (1 / sampled_tau)`: numpy returns the array itself for an exponent of 1.0
        q[j] = use_pow ? np_pow_as<F16>(p[j], tau_inv, use_pow) : p[j];
    }
    const float s2 = round_as<F16>(np_row_sum<T>(q, l, A, plan, lds));
    const bool nan_row = s != s;  // (the sum is every lane's: the whole row)
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int a = l + kWave * j;
        if (a < A) {
            probs[out_row * A + a] = nan_row ? np_softmax_nan<F16>(nan_any) : p[j];
            beta[out_row * A + a] = nan_row ? np_softmax_nan<F16>(nan_any) : round_as<F16>(q[j] / s2);
        }
    }
}

// The grid of k_policy_glue and k_root_glue is (B, R): root blockIdx.x, agent row blockIdx.y.  Row r
// takes the A logits (and legal entries) that start r * A past col_off (past the row's start) and is
// row blockIdx.x * R + r of the [B, R, A] noise and outputs.  R = 1 is one agent at col_off
// (mz_policy_glue, mz_root_glue and their _wide forms); R = N with col_off = 0 is every agent of a
// joint search in one launch (mz_policy_glue_joint, mz_root_glue_joint).
// Two things about the arguments of the glue kernels are there for the launch's cost.  R is an
// argument: reading gridDim would bring the hidden kernel arguments, 256 bytes more per dispatch, into
// the launch.  The sum plan comes in A's place (plan_len): the leading 14 dwords of arguments arrive
// preloaded in SGPRs (the build's kernarg preload), and one argument more, or a struct, which ends
// that sequence, would leave a fetch of 0.25 us in front of the first use of whatever falls behind.
template <bool F16, int T>
__global__ __launch_bounds__(kWave) void k_policy_glue(const void *logits, long long row_stride, long long col_off,
                                                       unsigned plan, int R, int use_pow, float tau_inv, float *probs,
                                                       float *beta, const unsigned short *hexp) {
    const int A = plan_len<T>(plan);
    __shared__ float lds[kWave * T];
    policy_glue_row<F16, T>(logits, row_stride, col_off + (long long)blockIdx.y * A, A, plan, use_pow, tau_inv, probs,
                            beta, hexp, blockIdx.x, (long long)blockIdx.x * R + blockIdx.y, threadIdx.x, lds);
}

// The current agent as per-row device state (the _rows entry points: rows of different agents in one
// launch).  Every lane reads the one word row_agent[t] and the value is made a scalar, so whatever
// depends on it -- the later agents' loop, the role test -- branches on SGPRs and the row bodies' ballots,
// wave_max and DPP butterflies stay in wave-uniform control flow, as with the launch constant.  A value
// outside [0, N) is clamped: no table indexes outside a logits row, a factor row or the later pool.
__device__ __forceinline__ int row_agent_of(const int *row_agent, int t, int N) {
    const int cur = __builtin_amdgcn_readfirstlane(row_agent[t]);
    return cur < 0 ? 0 : cur >= N ? N - 1 : cur;
}

// k_policy_glue for root blockIdx.x's own agent (grid (B)): the table's pointer stands where col_off
// stood and N where R stood, so the argument sequence and its preloaded part are k_policy_glue's.
template <bool F16, int T>
__global__ __launch_bounds__(kWave) void k_policy_glue_rows(const void *logits, long long row_stride,
                                                            const int *row_agent, unsigned plan, int N, int use_pow,
                                                            float tau_inv, float *probs, float *beta,
                                                            const unsigned short *hexp) {
    const int A = plan_len<T>(plan);
    __shared__ float lds[kWave * T];
    const int cur = row_agent_of(row_agent, blockIdx.x, N);
    policy_glue_row<F16, T>(logits, row_stride, (long long)cur * A, A, plan, use_pow, tau_inv, probs, beta, hexp,
                            blockIdx.x, blockIdx.x, threadIdx.x, lds);
}

// `x - m` of the root's softmax, m the row's maximum.  When m is a NaN numpy's result is a NaN operand
// as it stands (x's own where x is one), sign included; the GPU's subtraction negates its second
// operand first, a NaN's sign with it, so that case is picked by hand.
__device__ __forceinline__ float np_sub_max(float x, float m) {
    if (m != m) return (x != x) ? x : m;
    return x - m;
}

// Root preprocessing of mcts_sampled.py:64-100 for one (root, agent row) of the grid above (prepare's
// policy, beta and noise arguments, :102-106), with numpy 2.x's dtype rules (NEP 50):
//   probs = softmax(logits) in the logits' dtype                                       :64-65
//   legal (integer array): probs *= legal; probs += legal * 1e-4 (float64 arithmetic, stored in the
//     logits' dtype); probs /= sum(probs); noises (float32) likewise                     :73-83
//   beta = probs * (1 - eps) [logits' dtype] + noises * eps [float32] -> float32          :93
//   beta **= 1 / tau; beta *= legal (float64, stored float32); beta /= sum(beta)          :94-100
// `legal` holds int32 rows (the caller checked the integer array's values fit), or is null.  The
// Dirichlet noise is drawn by the caller (np_random order) and arrives as float32.  A row that holds
// a NaN keeps it through np.max and np_sub_max; such rows and rows with an infinite maximum are not
// pinned against numpy.
template <bool F16, int T>
__global__ __launch_bounds__(kWave) void k_root_glue(const void *logits, long long row_stride, long long col_off,
                                                     unsigned plan, int R, const int *legal, long long legal_stride,
                                                     const float *noise_in, double one_minus_eps, double eps,
                                                     int use_pow, float tau_inv, float *probs, float *beta,
                                                     float *noise_out, const unsigned short *hexp) {
    const int A = plan_len<T>(plan);
    __shared__ float lds[kWave * T];
    const int t = blockIdx.x;
    const int l = threadIdx.x;
    const long long agent_off = (long long)blockIdx.y * A, out = ((long long)t * R + blockIdx.y) * A;
    float x[T], p[T], n[T], b[T];
    double lg[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int a = l + kWave * j;
        x[j] = a < A ? load_elem<F16>(logits, (long long)t * row_stride + col_off + agent_off + a) : -INFINITY;
        n[j] = a < A ? noise_in[out + a] : 0.f;
        lg[j] = (legal && a < A) ? (double)legal[(long long)t * legal_stride + agent_off + a] : 0.0;
    }
    const float m = np_row_max<T>(x, l, A);
#pragma unroll
    for (int j = 0; j < T; ++j) p[j] = np_exp_as<F16>(round_as<F16>(np_sub_max(x[j], m)), hexp);
    const float s = round_as<F16>(np_row_sum<T>(p, l, A, plan, lds));
#pragma unroll
    for (int j = 0; j < T; ++j) p[j] = round_as<F16>(p[j] / s);
    if (legal) {
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const double tiny = lg[j] * 1e-4;  // `legal * 1e-4`: a float64 array
            p[j] = store_d<F16>((double)p[j] * lg[j]);
            p[j] = store_d<F16>((double)p[j] + tiny);
            n[j] = (float)((double)n[j] * lg[j]);
            n[j] = (float)((double)n[j] + tiny);
        }
        const float sp = round_as<F16>(np_row_sum<T>(p, l, A, plan, lds));
        const float sn = np_row_sum<T>(n, l, A, plan, lds);
#pragma unroll
        for (int j = 0; j < T; ++j) {
            p[j] = round_as<F16>(p[j] / sp);
            n[j] = n[j] / sn;
        }
    }
    // probs * (1 - eps): the Python float becomes the array's dtype (NEP 50); noises * eps in float32;
    // the sum of a half and a float32 array is float32
    const float c1 = store_d<F16>(one_minus_eps), c2 = (float)eps;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const float a1 = round_as<F16>(p[j] * c1);
        b[j] = a1 + n[j] * c2;
        if (use_pow) b[j] = np_pow_as<false>(b[j], tau_inv, use_pow);  // a float32 array
        if (legal) b[j] = (float)((double)b[j] * lg[j]);
    }
    const float sb = np_row_sum<T>(b, l, A, plan, lds);
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int a = l + kWave * j;
        if (a < A) {
            probs[out + a] = p[j];
            beta[out + a] = b[j] / sb;
            noise_out[out + a] = n[j];
        }
    }
}

// mcts_sampled.py:116-147 for root blockIdx.x: previous agents from `factor`, the current agent
// from the selection, the following agents by numpy argmax of the leaf policy logits.  `cur` is
// wave-uniform (np_argmax_row's ballots): the launch's agent, or the root's own (k_joint_action_rows).
template <bool F16, int T>
__device__ __forceinline__ void joint_action_row(const void *pred, int N, int A, int cur, const int *factor, int fcols,
                                                 const int *actions, long long *joint) {
    const int t = blockIdx.x;
    const int l = threadIdx.x;
    if (l < N && l <= cur) joint[(long long)t * N + l] = (l < cur) ? (long long)factor[(long long)t * fcols + l]
                                                                    : (long long)actions[t];
    for (int k = cur + 1; k < N; ++k) {
        const int idx = np_argmax_row<F16, T>(pred, ((long long)t * N + k) * A, A, l);
        if (l == 0) joint[(long long)t * N + k] = idx;
    }
}

template <bool F16, int T>
__global__ __launch_bounds__(kWave) void k_joint_action(const void *pred, int N, int A, int cur, const int *factor,
                                                        int fcols, const int *actions, long long *joint) {
    joint_action_row<F16, T>(pred, N, A, cur, factor, fcols, actions, joint);
}

template <bool F16, int T>
__global__ __launch_bounds__(kWave) void k_joint_action_rows(const void *pred, int N, int A, const int *row_agent,
                                                             const int *factor, int fcols, const int *actions,
                                                             long long *joint) {
    joint_action_row<F16, T>(pred, N, A, row_agent_of(row_agent, blockIdx.x, N), factor, fcols, actions, joint);
}

// mz_policy_glue_later: one wave per (root, role), grid (B, roles).  Role 0 is the policy glue of the
// current agent (absent when the caller wants the later agents only: then `glue` is 0 and every role
// is an argmax); role j >= 1 is np.argmax of agent cur + j's logits into later[t, cur + j].  The role
// is the workgroup's, so the ballots and wave_max of either body stay in wave-uniform control flow.
constexpr int kMaxGridRows = 65535;  // grid.y: a role per agent here, an agent per row in the joint glue
template <bool F16, int T>
__global__ __launch_bounds__(kWave) void k_policy_glue_later(const void *logits, long long row_stride, int N, unsigned plan,
                                                             int cur, int glue, int use_pow, float tau_inv,
                                                             float *probs, float *beta, int *later,
                                                             const unsigned short *hexp) {
    const int A = plan_len<T>(plan);
    __shared__ float lds[kWave * T];
    const int t = blockIdx.x;
    const int l = threadIdx.x;
    const int j = (int)blockIdx.y + 1 - glue;
    if (j == 0) {
        policy_glue_row<F16, T>(logits, row_stride, (long long)cur * A, A, plan, use_pow, tau_inv, probs, beta, hexp, t,
                                t, l, lds);
        return;
    }
    const int k = cur + j;
    const int idx = np_argmax_row<F16, T>(logits, (long long)t * row_stride + (long long)k * A, A, l);
    if (l == 0) later[(long long)t * N + k] = idx;
}

// k_policy_glue_later with root t's own agent, grid (B, glue + N - 1): every root gets the roles of
// agent 0, and the workgroups of a role past the root's last agent return at once.
template <bool F16, int T>
__global__ __launch_bounds__(kWave) void k_policy_glue_later_rows(const void *logits, long long row_stride,
                                                                  const int *row_agent, unsigned plan, int N, int glue,
                                                                  int use_pow, float tau_inv, float *probs,
                                                                  float *beta, int *later,
                                                                  const unsigned short *hexp) {
    const int A = plan_len<T>(plan);
    __shared__ float lds[kWave * T];
    const int t = blockIdx.x;
    const int l = threadIdx.x;
    const int cur = row_agent_of(row_agent, t, N);
    const int j = (int)blockIdx.y + 1 - glue;
    if (j == 0) {
        policy_glue_row<F16, T>(logits, row_stride, (long long)cur * A, A, plan, use_pow, tau_inv, probs, beta, hexp, t,
                                t, l, lds);
        return;
    }
    const int k = cur + j;
    if (k >= N) return;  // (the workgroup's: cur and j are scalars)
    const int idx = np_argmax_row<F16, T>(logits, (long long)t * row_stride + (long long)k * A, A, l);
    if (l == 0) later[(long long)t * N + k] = idx;
}

// mz_joint_action_cached: one thread per (root i, agent k); the later agents' actions are those the
// node selected for root i (its hidden_state_index_x, idx_x[i]) got from mz_policy_glue_later.
constexpr int kCachedLanes = 256;
// element e = (root i, agent k) of the joint action; cur is root i's agent
__device__ __forceinline__ void joint_action_cached_elem(const int *pool, int slots, const int *idx_x, int B, int N,
                                                         int cur, const int *factor, int fcols, const int *actions,
                                                         long long *joint, long long e) {
    const int i = (int)(e / N), k = (int)(e % N);
    long long v;
    if (k < cur) {
        v = factor[(long long)i * fcols + k];
    } else if (k == cur) {
        v = actions[i];
    } else {
        int s = idx_x[i];
        if (s < 0 || s >= slots) s = 0;  // (never outside the pool: the joint action feeds an embedding)
        v = pool[((long long)s * B + i) * N + k];
    }
    joint[e] = v;
}

__global__ __launch_bounds__(kCachedLanes) void k_joint_action_cached(const int *pool, int slots, const int *idx_x,
                                                                      int B, int N, int cur, const int *factor,
                                                                      int fcols, const int *actions,
                                                                      long long *joint) {
    const long long e = (long long)blockIdx.x * kCachedLanes + threadIdx.x;
    if (e >= (long long)B * N) return;
    joint_action_cached_elem(pool, slots, idx_x, B, N, cur, factor, fcols, actions, joint, e);
}

// k_joint_action_cached with root i's own agent, clamped to [0, N - 1] as the slot is (a lane's own
// value: nothing here is a wave operation)
__global__ __launch_bounds__(kCachedLanes) void k_joint_action_cached_rows(const int *pool, int slots, const int *idx_x,
                                                                           int B, int N, const int *row_agent,
                                                                           const int *factor, int fcols,
                                                                           const int *actions, long long *joint) {
    const long long e = (long long)blockIdx.x * kCachedLanes + threadIdx.x;
    if (e >= (long long)B * N) return;
    int cur = row_agent[e / N];
    cur = cur < 0 ? 0 : cur >= N ? N - 1 : cur;
    joint_action_cached_elem(pool, slots, idx_x, B, N, cur, factor, fcols, actions, joint, e);
}

// ------------------------------------------------------------------------------------------------
// Inverse support transform of the value and reward heads (core/config.py:430-499 after
// config/smac/model.py:562-572): softmax -> _inv_phi -> _inv_h.  The target is not numpy but the
// torch chain on this device (mazero_amd.nets.inverse_support_transform under autocast), restated
// from the kernels torch launches for it:
//   softmax   softmax_warp_forward (ATen PersistentSoftmax.cuh): next_pow2(S) lanes, one element per
//             lane for S <= 64, pad lanes at -inf; max `a < b ? b : a` and the sum as xor butterflies
//             from width / 2 down to 1, every lane keeping its own result (a NaN does not spread
//             through the max, so lanes may hold different maxima; the sum spreads it); ::exp;
//             NaN in every element when the sum is 0
//   mul       float(support) * p, one f32 multiply
//   sum       ATen Reduce.cuh for fewer than 128 inputs per output: block width bw = last_pow2(S);
//             thread x adds elements x and x + bw to accumulators 0 and 1 of four that start at 0,
//             joins them ((v0 + v1) + v2) + v3, then lane x takes lane x + offset for offset = 1, 2,
//             .. < bw; the row's sum is lane 0's
//   _inv_h    one f32 kernel per Python operator, Python scalars cast to f32; a tensor divided by a
//             Python scalar is multiplied by the scalar's reciprocal (double, cast to f32)
// This translation unit is built without FMA contraction and with IEEE divide and sqrt.
constexpr int kInvWaves = 4;  // waves per workgroup of k_inverse_rows
constexpr int kInvLanes = 256;
constexpr int kInvMaxGrid = 1 << 20;
constexpr float kInvEps = (float)0.001;
constexpr float kInv4Eps = (float)(4 * 0.001);
// `/ (2 * epsilon)`: torch multiplies by the reciprocal, taken in double and then cast (500.0f; the
// f32 reciprocal of f32(0.002) would be 499.99997f)
constexpr float kInvHalfOverEps = (float)(1.0 / (2 * 0.001));

struct InvHead {
    const void *in;
    float *out;
    long long stride;  // elements between rows
    int lo, S;         // the support is lo .. lo + S - 1
    int f16;
};

__device__ __forceinline__ float torch_inv_h(float x) {
    float a = fabsf(x) + 1.0f;
    a = a + kInvEps;
    a = kInv4Eps * a;
    a = 1.0f + a;
    a = sqrtf(a);  // (IEEE: -fhip-fp32-correctly-rounded-divide-sqrt)
    a = a - 1.0f;
    a = a * kInvHalfOverEps;
    a = a * a;
    a = a - 1.0f;
    float out = (x < 0.f ? -1.0f : 1.0f) * a;
    if (out != out) out = 0.f;
    if (fabsf(out) < kInvEps) out = 0.f;
    return out;
}

// One wave per (row, head), lane l holds support element l; blockIdx.y is the head.
__global__ __launch_bounds__(kInvLanes) void k_inverse_rows(InvHead h0, InvHead h1, int n, int probs) {
    const InvHead h = blockIdx.y ? h1 : h0;
    const int l = threadIdx.x & (kWave - 1);
    const int S = h.S;
    int W = 1, bw = 1;  // next_pow2(S), last_pow2(S)
    while (W < S) W <<= 1;
    while (2 * bw <= S) bw <<= 1;
    const bool on = l < S;
    for (long long row = (long long)blockIdx.x * kInvWaves + (threadIdx.x >> 6); row < n;
         row += (long long)gridDim.x * kInvWaves) {
        float p;
        if (probs) {
            p = on ? static_cast<const float *>(h.in)[row * h.stride + l] : 0.f;
        } else {
            float x = -INFINITY;
            if (on) x = h.f16 ? load_elem<true>(h.in, row * h.stride + l) : load_elem<false>(h.in, row * h.stride + l);
            float m = x;
            for (int o = W >> 1; o > 0; o >>= 1) {
                const float b = __shfl_xor(m, o, kWave);
                m = m < b ? b : m;
            }
            const float e = ::expf(x - m);
            float s = 0.0f + e;
            for (int o = W >> 1; o > 0; o >>= 1) s = s + __shfl_xor(s, o, kWave);
            p = (s == 0.f) ? NAN : e / s;
        }
        const float q = on ? (float)(h.lo + l) * p : 0.f;
        const float q2 = bw < kWave ? __shfl_down(q, bw, kWave) : 0.f;
        const float v0 = 0.0f + q;
        const float v1 = (l + bw < S) ? 0.0f + q2 : 0.0f;
        float acc = ((v0 + v1) + 0.0f) + 0.0f;
        for (int o = 1; o < bw; o <<= 1) acc = acc + __shfl_down(acc, o, kWave);
        if (l == 0) h.out[row] = torch_inv_h(acc);
    }
}

// MZ_INV_EXPECTATION: one lane per (row, head)
__global__ __launch_bounds__(kInvLanes) void k_inverse_scalars(InvHead h0, InvHead h1, int n) {
    const InvHead h = blockIdx.y ? h1 : h0;
    for (long long i = (long long)blockIdx.x * kInvLanes + threadIdx.x; i < n; i += (long long)gridDim.x * kInvLanes)
        h.out[i] = torch_inv_h(static_cast<const float *>(h.in)[i * h.stride]);
}

// ------------------------------------------------------------------------------------------------
// The same chain for supports of 65 .. 1024 elements (the reference's default [-300, 300] is 601),
// again restated from the kernels torch launches:
//   softmax   softmax_warp_forward with W = next_pow2(S) / 64 elements per lane: lane l holds elements
//             l + 64 it, elements past S at -inf; the lane's own maximum first, `m > x ? m : x` in it
//             order (a NaN survives only as the last element), then the butterfly of k_inverse_rows
//             (`m < b ? b : m`, 32 .. 1); ::exp; the lane's sum from 0.0f in it order, pad elements
//             included, then the xor-add butterfly; NaN in every element when the sum is 0
//   mul       float(support) * p, one f32 multiply, into a fresh contiguous [n, S] tensor
//   sum       ATen Reduce.cuh over that tensor.  65 <= S < 128: block width 64, thread x adds elements x
//             and x + 64 to accumulators 0 and 1 of four, as in k_inverse_rows.  S >= 128 ("vectorize
//             along input"): the row is read as 16-byte-aligned vectors of 4 floats, so the order
//             depends on the row's misalignment shift = (row * S) % 4: threads shift <= x < 4 first take
//             row element x - shift into accumulator 0 (shift > 0), thread x then adds the aligned
//             vectors x, x + bw, .. component i to accumulator i, threads x < 4 add the tail element to
//             accumulator 0; join ((v0 + v1) + v2) + v3.  The block width bw (32 .. 256) follows from
//             S and from the row count n (ReduceConfig::set_block_dimension; inverse_sum_plan below).
//             Threads past 64 are folded through shared memory, t[x] += t[x + off] for off = bw / 2 ..
//             64, then lane x takes lane x + off for off = 1, 2, .. < min(bw, 64).
// One wave per (row, head) as in k_inverse_rows.  The products go through a row of LDS that only this
// wave touches, placed at offset `shift` so that torch's vector loads are aligned LDS reads; lane l
// plays torch's threads l, l + 64, l + 128, l + 192 in turn, so the shared-memory folds are adds
// within the lane.  IT >= the elements per lane of either head (the elements stay in registers).
// On the MI355X all of this held as derived from the installed torch's headers: bit-identical to the
// torch chain for 16 support sizes from 65 to 1024, row counts on both sides of every block-width
// switch, all four row alignments, f32 and f16 logits (tests/test_inverse_transform_wide.py); nothing
// had to be corrected and no regime is refused.
constexpr int kInvWideMax = 1024;            // softmax_warp_forward's limit
constexpr int kInvWideRow = kInvWideMax + 4;  // + one vector: the row starts at offset shift <= 3

struct InvPlan {
    int vec;  // 1: "vectorize along input" (S >= 128)
    int bw;   // torch's block width
    int nit;  // next_pow2(S) / 64: the softmax's elements per lane
};

// what torch's thread x of bw sums of the row q[0 .. S) stored at d[shift ..] (d 16-byte aligned)
__device__ __forceinline__ float torch_vec_thread_sum(const float *d, int S, int shift, int x, int bw) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    int end = S;
    if (shift > 0) {
        if (x >= shift && x < 4) a0 = a0 + d[x];
        end = S + shift - 4;
        d += 4;
    }
    for (int v = x; 4 * v + 3 < end; v += bw) {
        const float4 t = *reinterpret_cast<const float4 *>(d + 4 * v);
        a0 = a0 + t.x;
        a1 = a1 + t.y;
        a2 = a2 + t.z;
        a3 = a3 + t.w;
    }
    const int tail = end - end % 4 + x;
    if (tail < end) a0 = a0 + d[tail];
    return ((a0 + a1) + a2) + a3;
}

template <int IT>
__global__ __launch_bounds__(kInvLanes) void k_inverse_rows_wide(InvHead h0, InvHead h1, InvPlan p0, InvPlan p1, int n,
                                                                  int probs) {
    __shared__ __attribute__((aligned(16))) float rows[kInvWaves][kInvWideRow];
    const InvHead h = blockIdx.y ? h1 : h0;
    const InvPlan plan = blockIdx.y ? p1 : p0;
    const int l = threadIdx.x & (kWave - 1);
    float *lds = rows[threadIdx.x >> 6];
    const int S = h.S, nit = plan.nit, bw = plan.bw;
    for (long long row = (long long)blockIdx.x * kInvWaves + (threadIdx.x >> 6); row < n;
         row += (long long)gridDim.x * kInvWaves) {
        const long long base = row * h.stride;
        float e[IT];  // logits, exponentials, probabilities, then support * p of elements l + 64 it
        if (probs) {
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int idx = l + kWave * it;
                e[it] = idx < S ? static_cast<const float *>(h.in)[base + idx] : 0.f;
            }
        } else {
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int idx = l + kWave * it;
                e[it] = -INFINITY;
                if (idx < S) e[it] = h.f16 ? load_elem<true>(h.in, base + idx) : load_elem<false>(h.in, base + idx);
            }
            float m = e[0];
#pragma unroll
            for (int it = 0; it < IT; ++it)
                if (it < nit) m = m > e[it] ? m : e[it];
            for (int o = kWave >> 1; o > 0; o >>= 1) {
                const float b = __shfl_xor(m, o, kWave);
                m = m < b ? b : m;
            }
            float s = 0.0f;
#pragma unroll
            for (int it = 0; it < IT; ++it)
                if (it < nit) {
                    e[it] = ::expf(e[it] - m);
                    s = s + e[it];
                }
            for (int o = kWave >> 1; o > 0; o >>= 1) s = s + __shfl_xor(s, o, kWave);
#pragma unroll
            for (int it = 0; it < IT; ++it) e[it] = (s == 0.f) ? NAN : e[it] / s;
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = l + kWave * it;
            e[it] = idx < S ? (float)(h.lo + idx) * e[it] : 0.f;
        }
        float acc;
        if (!plan.vec) {  // 65 <= S < 128: bw = 64, elements l and l + 64 are this lane's own
            const float v0 = 0.0f + e[0];
            const float v1 = (l + kWave < S) ? 0.0f + e[1] : 0.0f;
            acc = ((v0 + v1) + 0.0f) + 0.0f;
        } else {
            const int shift = (int)((row * S) & 3);
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int idx = l + kWave * it;
                if (idx < S) lds[shift + idx] = e[it];
            }
            // the row is this wave's alone: its LDS writes have landed once the counter drains
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = l + kWave * k;
                if (x < bw) t[k] = torch_vec_thread_sum(lds, S, shift, x, bw);
            }
            if (bw == 256)
                acc = (t[0] + t[2]) + (t[1] + t[3]);
            else if (bw == 128)
                acc = t[0] + t[1];
            else
                acc = t[0];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (read before the next row overwrites it)
        }
        const int width = bw < kWave ? bw : kWave;
        for (int o = 1; o < width; o <<= 1) acc = acc + __shfl_down(acc, o, kWave);
        if (l == 0) h.out[row] = torch_inv_h(acc);
    }
}

// ReduceConfig::set_block_dimension for torch.sum over the last dimension of a contiguous float32
// [n, S] tensor (MAX_NUM_THREADS 512, input_vec_size 4, wave 64)
static int last_pow2_int(int64_t v) {
    int p = 1;
    while (2 * (int64_t)p <= v) p <<= 1;
    return p;
}

static void inverse_sum_plan(int S, int n, int *vectorized, int *block_width) {
    constexpr int kMaxThreads = 512;
    int64_t dim0 = S;
    *vectorized = S >= 128;
    if (*vectorized) dim0 /= 4;
    const int d0 = dim0 < kMaxThreads ? last_pow2_int(dim0) : kMaxThreads;
    const int d1 = n < kMaxThreads ? last_pow2_int(n) : kMaxThreads;
    int w = d0 < kWave ? d0 : kWave;
    const int hgt = d1 < kMaxThreads / w ? d1 : kMaxThreads / w;
    w = d0 < kMaxThreads / hgt ? d0 : kMaxThreads / hgt;
    *block_width = w;
}

// the table of mz_set_half_exp_table per device (allocated once, never freed: captured graphs keep
// its address)
constexpr int kMaxDevices = 64;
unsigned short *g_half_exp[kMaxDevices];
std::mutex g_half_exp_mu;

// the current device's table (the launchers call this after making the handle's device current)
const unsigned short *half_exp_table() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
    std::lock_guard<std::mutex> lk(g_half_exp_mu);
    return g_half_exp[dev];
}

// ------------------------------------------------------------------------------------------------
// What the glue launchers share.  `fn` names the entry point in the messages.  Every entry point
// checks its arguments in an order of its own, so the shared steps are separate calls.
int glue_fail(int code, const char *fn, const char *what) {
    return mz_internal_fail(code, (std::string(fn) + ": " + what).c_str());
}

struct Glue {
    const char *fn;
    mz_batch *b;
    int B = 0, A = 0;
    hipStream_t stream = nullptr;
    unsigned plan = 0u;  // sum_plan(A)
    int use_pow = 0;     // `** (1 / sampled_tau)`: pow_mode and the exponent as numpy casts it
    float tau_inv = 1.f;
    const unsigned short *hexp = nullptr;
};

// the handle's device current, its B, A and stream
int glue_handle(Glue *g, const char *fn, mz_batch *b) {
    g->fn = fn;
    g->b = b;
    return mz_internal_launch_info(b, &g->B, &g->A, &g->stream);
}

// glue_handle for an entry point that reads rows of A actions: A within its bound, one lane per action,
// or with `wide` every A the handle has (the kernels are the same, include/mzdriver.h)
int glue_begin(Glue *g, const char *fn, mz_batch *b, bool wide) {
    if (int rc = glue_handle(g, fn, b)) return rc;
    if (!wide && g->A > kWave) return glue_fail(MZ_ERR_UNSUPPORTED, fn, "action_space_size > 64");
    if (g->A > kWideMax) return glue_fail(MZ_ERR_UNSUPPORTED, fn, "action_space_size > 255");
    g->plan = sum_plan(g->A);
    return MZ_OK;
}

int glue_dtype(const Glue &g, int dtype) {
    if (dtype != MZ_DT_F32 && dtype != MZ_DT_F16) return glue_fail(MZ_ERR_ARG, g.fn, "bad dtype");
    return MZ_OK;
}

// Python's `1 / sampled_tau`, cast to the dtype of the array it raises (NEP 50): the logits' for the
// policy glue (`half`: float16), float32 for the root's beta; and the softmax's half-exp table
int glue_tau(Glue *g, double sampled_tau, bool half) {
    if (!(sampled_tau > 0.0)) return glue_fail(MZ_ERR_ARG, g->fn, "sampled_tau must be > 0");
    const double inv = 1.0 / sampled_tau;
    g->tau_inv = half ? (float)(_Float16)inv : (float)inv;
    g->use_pow = pow_mode(inv);
    g->hexp = half_exp_table();
    return MZ_OK;
}

// (dtype, A) -> <F16, T = ceil(A / 64)>: launch(std::bool_constant<F16>, std::integral_constant<int, T>)
template <class Launch>
void glue_dispatch(int dtype, int A, Launch launch) {
    auto tiles = [&](auto f16) {
        switch ((A + kWave - 1) / kWave) {
            case 1: launch(f16, std::integral_constant<int, 1>{}); break;
            case 2: launch(f16, std::integral_constant<int, 2>{}); break;
            case 3: launch(f16, std::integral_constant<int, 3>{}); break;
            default: launch(f16, std::integral_constant<int, 4>{}); break;
        }
    };
    if (dtype == MZ_DT_F16)
        tiles(std::true_type{});
    else
        tiles(std::false_type{});
}

int glue_end(const Glue &g) {
    mz_internal_enqueued(g.b);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mz_internal_fail(MZ_ERR_DEVICE, hipGetErrorString(e));
    return MZ_OK;
}

// k_policy_glue / k_root_glue on a grid of (B, rows)
int launch_policy_glue(const Glue &g, int dtype, int rows, const void *logits, int64_t row_stride,
                       int64_t col_offset, float *probs_out, float *beta_out) {
    glue_dispatch(dtype, g.A, [&](auto f16, auto tiles) {
        hipLaunchKernelGGL((k_policy_glue<decltype(f16)::value, decltype(tiles)::value>), dim3(g.B, rows),
                           dim3(kWave), 0, g.stream, logits, (long long)row_stride, (long long)col_offset, g.plan, rows,
                           g.use_pow, g.tau_inv, probs_out, beta_out, g.hexp);
    });
    return glue_end(g);
}

int launch_root_glue(const Glue &g, int dtype, int rows, const void *logits, int64_t row_stride, int64_t col_offset,
                     const int32_t *legal, int64_t legal_stride, const float *noises, double noise_eps,
                     float *probs_out, float *beta_out, float *noises_out) {
    const double ome = 1.0 - noise_eps;  // (Python float arithmetic)
    glue_dispatch(dtype, g.A, [&](auto f16, auto tiles) {
        hipLaunchKernelGGL((k_root_glue<decltype(f16)::value, decltype(tiles)::value>), dim3(g.B, rows), dim3(kWave),
                           0, g.stream, logits, (long long)row_stride, (long long)col_offset, g.plan, rows,
                           (const int *)legal, (long long)legal_stride, noises, ome, noise_eps, g.use_pow,
                           g.tau_inv, probs_out, beta_out, noises_out, g.hexp);
    });
    return glue_end(g);
}

}  // namespace

extern "C" {

int mz_set_half_exp_table(const uint16_t *table) {
    if (!table) return mz_internal_fail(MZ_ERR_ARG, "mz_set_half_exp_table: null table");
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return mz_internal_fail(MZ_ERR_DEVICE, hipGetErrorString(e));
    if (dev < 0 || dev >= kMaxDevices) return mz_internal_fail(MZ_ERR_UNSUPPORTED, "mz_set_half_exp_table: device id");
    std::lock_guard<std::mutex> lk(g_half_exp_mu);
    if (!g_half_exp[dev]) {
        void *p = nullptr;
        e = hipMalloc(&p, 65536 * sizeof(uint16_t));
        if (e != hipSuccess) return mz_internal_fail(MZ_ERR_DEVICE, hipGetErrorString(e));
        g_half_exp[dev] = (unsigned short *)p;
    }
    e = hipMemcpy(g_half_exp[dev], table, 65536 * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return mz_internal_fail(MZ_ERR_DEVICE, hipGetErrorString(e));
    return MZ_OK;
}

// mz_policy_glue, mz_root_glue, mz_joint_action and their _wide forms (`wide`: any A the handle has)
static int policy_glue(const char *fn, bool wide, mz_batch *b, const void *logits, int dtype, int64_t row_stride,
                       int64_t col_offset, double sampled_tau, float *probs_out, float *beta_out) {
    Glue g;
    if (int rc = glue_begin(&g, fn, b, wide)) return rc;
    if (!logits || !probs_out || !beta_out) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (int rc = glue_dtype(g, dtype)) return rc;
    if (row_stride < g.A || col_offset < 0 || col_offset + g.A > row_stride)
        return glue_fail(MZ_ERR_ARG, fn, "logits row does not hold the agent's actions");
    if (int rc = glue_tau(&g, sampled_tau, dtype == MZ_DT_F16)) return rc;
    return launch_policy_glue(g, dtype, 1, logits, row_stride, col_offset, probs_out, beta_out);
}

static int root_glue(const char *fn, bool wide, mz_batch *b, const void *logits, int dtype, int64_t row_stride,
                     int64_t col_offset, const int32_t *legal, int64_t legal_stride, const float *noises,
                     double noise_eps, double sampled_tau, float *probs_out, float *beta_out, float *noises_out) {
    Glue g;
    if (int rc = glue_begin(&g, fn, b, wide)) return rc;
    if (!logits || !noises || !probs_out || !beta_out || !noises_out) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (int rc = glue_dtype(g, dtype)) return rc;
    if (row_stride < g.A || col_offset < 0 || col_offset + g.A > row_stride)
        return glue_fail(MZ_ERR_ARG, fn, "logits row does not hold the agent's actions");
    if (legal && legal_stride < g.A) return glue_fail(MZ_ERR_ARG, fn, "legal rows hold fewer than A");
    if (int rc = glue_tau(&g, sampled_tau, false)) return rc;  // beta is a float32 array here (:93)
    return launch_root_glue(g, dtype, 1, logits, row_stride, col_offset, legal, legal_stride, noises, noise_eps,
                            probs_out, beta_out, noises_out);
}

static int joint_action(const char *fn, bool wide, mz_batch *b, const void *pred_logits, int dtype, int num_agents,
                        int current_agent, const int32_t *factor, int factor_cols, const int32_t *actions,
                        int64_t *joint_out) {
    Glue g;
    if (int rc = glue_begin(&g, fn, b, wide)) return rc;
    if (num_agents < 1 || num_agents > kWave || current_agent < 0 || current_agent >= num_agents)
        return glue_fail(MZ_ERR_ARG, fn, "bad agent index / count");
    if (!actions || !joint_out) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (current_agent > 0 && (!factor || factor_cols < current_agent))
        return glue_fail(MZ_ERR_ARG, fn, "factor must hold the previous agents' actions");
    if (current_agent + 1 < num_agents && !pred_logits)
        return glue_fail(MZ_ERR_ARG, fn, "leaf policy logits required for later agents");
    if (int rc = glue_dtype(g, dtype)) return rc;
    glue_dispatch(dtype, g.A, [&](auto f16, auto tiles) {
        hipLaunchKernelGGL((k_joint_action<decltype(f16)::value, decltype(tiles)::value>), dim3(g.B), dim3(kWave), 0,
                           g.stream, pred_logits, num_agents, g.A, current_agent, (const int *)factor, factor_cols,
                           (const int *)actions, (long long *)joint_out);
    });
    return glue_end(g);
}

int mz_policy_glue_later(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int num_agents,
                         int current_agent, double sampled_tau, float *probs_out, float *beta_out,
                         int32_t *later_out) {
    const char *fn = "mz_policy_glue_later";
    Glue g;
    if (int rc = glue_begin(&g, fn, b, true)) return rc;
    if (num_agents < 1 || num_agents > kMaxGridRows || current_agent < 0 || current_agent >= num_agents)
        return glue_fail(MZ_ERR_ARG, fn, "bad agent index / count");
    if (!logits) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (!probs_out != !beta_out) return glue_fail(MZ_ERR_ARG, fn, "probs_out and beta_out go together");
    const int glue = probs_out ? 1 : 0, later = num_agents - 1 - current_agent;
    if (later > 0 && !later_out) return glue_fail(MZ_ERR_ARG, fn, "later_out required for later agents");
    if (glue + later == 0) return glue_fail(MZ_ERR_ARG, fn, "no output asked for");
    if (int rc = glue_dtype(g, dtype)) return rc;
    if (row_stride < (int64_t)num_agents * g.A)
        return glue_fail(MZ_ERR_ARG, fn, "logits row does not hold every agent's actions");
    if (int rc = glue_tau(&g, sampled_tau, dtype == MZ_DT_F16)) return rc;  // as mz_policy_glue
    glue_dispatch(dtype, g.A, [&](auto f16, auto tiles) {
        hipLaunchKernelGGL((k_policy_glue_later<decltype(f16)::value, decltype(tiles)::value>),
                           dim3(g.B, glue + later), dim3(kWave), 0, g.stream, logits, (long long)row_stride,
                           num_agents, g.plan, current_agent, glue, g.use_pow, g.tau_inv, probs_out, beta_out,
                           (int *)later_out, g.hexp);
    });
    return glue_end(g);
}

int mz_joint_action_cached(mz_batch *b, const int32_t *later_pool, int slots, const int32_t *idx_x, int num_agents,
                           int current_agent, const int32_t *factor, int factor_cols, const int32_t *actions,
                           int64_t *joint_out) {
    const char *fn = "mz_joint_action_cached";
    Glue g;
    if (int rc = glue_handle(&g, fn, b)) return rc;  // (any A: no row of actions is read)
    if (num_agents < 1 || num_agents > kMaxGridRows || current_agent < 0 || current_agent >= num_agents)
        return glue_fail(MZ_ERR_ARG, fn, "bad agent index / count");
    if (!actions || !joint_out) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (current_agent > 0 && (!factor || factor_cols < current_agent))
        return glue_fail(MZ_ERR_ARG, fn, "factor must hold the previous agents' actions");
    if (current_agent + 1 < num_agents && (!later_pool || !idx_x || slots < 1))
        return glue_fail(MZ_ERR_ARG, fn, "later-action pool and idx_x required for later agents");
    const long long n = (long long)g.B * num_agents;
    hipLaunchKernelGGL(k_joint_action_cached, dim3((unsigned)((n + kCachedLanes - 1) / kCachedLanes)),
                       dim3(kCachedLanes), 0, g.stream, (const int *)later_pool, slots, (const int *)idx_x, g.B,
                       num_agents, current_agent, (const int *)factor, factor_cols, (const int *)actions,
                       (long long *)joint_out);
    return glue_end(g);
}

// The _rows entry points: the current agent from a device table, one entry per root.  The launchers
// cannot see the table (the kernels clamp what it holds); what they check is what every agent needs.
static int rows_agents(const Glue &g, int num_agents, int max_agents, const int32_t *row_agent) {
    if (num_agents < 1 || num_agents > max_agents) return glue_fail(MZ_ERR_ARG, g.fn, "bad agent count");
    if (!row_agent) return glue_fail(MZ_ERR_ARG, g.fn, "null row_agent");
    return MZ_OK;
}

// factor [B, factor_cols]: a row of agent N - 1 reads N - 1 columns (none with one agent)
static int rows_factor(const Glue &g, int num_agents, const int32_t *factor, int factor_cols) {
    if (factor_cols < (num_agents > 2 ? num_agents - 1 : 1))
        return glue_fail(MZ_ERR_ARG, g.fn, "factor_cols < max(1, num_agents - 1)");
    if (num_agents > 1 && !factor) return glue_fail(MZ_ERR_ARG, g.fn, "factor must hold the previous agents' actions");
    return MZ_OK;
}

int mz_policy_glue_rows(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int num_agents,
                        const int32_t *row_agent, double sampled_tau, float *probs_out, float *beta_out) {
    const char *fn = "mz_policy_glue_rows";
    Glue g;
    if (int rc = glue_begin(&g, fn, b, true)) return rc;
    if (int rc = rows_agents(g, num_agents, kMaxGridRows, row_agent)) return rc;
    if (!logits || !probs_out || !beta_out) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (int rc = glue_dtype(g, dtype)) return rc;
    if (row_stride < (int64_t)num_agents * g.A)
        return glue_fail(MZ_ERR_ARG, fn, "logits row does not hold every agent's actions");
    if (int rc = glue_tau(&g, sampled_tau, dtype == MZ_DT_F16)) return rc;  // as mz_policy_glue
    glue_dispatch(dtype, g.A, [&](auto f16, auto tiles) {
        hipLaunchKernelGGL((k_policy_glue_rows<decltype(f16)::value, decltype(tiles)::value>), dim3(g.B), dim3(kWave),
                           0, g.stream, logits, (long long)row_stride, (const int *)row_agent, g.plan, num_agents,
                           g.use_pow, g.tau_inv, probs_out, beta_out, g.hexp);
    });
    return glue_end(g);
}

int mz_joint_action_rows(mz_batch *b, const void *pred_logits, int dtype, int num_agents, const int32_t *row_agent,
                         const int32_t *factor, int factor_cols, const int32_t *actions, int64_t *joint_out) {
    const char *fn = "mz_joint_action_rows";
    Glue g;
    if (int rc = glue_begin(&g, fn, b, true)) return rc;
    if (int rc = rows_agents(g, num_agents, kWave, row_agent)) return rc;  // (a lane per earlier agent)
    if (!actions || !joint_out) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (int rc = rows_factor(g, num_agents, factor, factor_cols)) return rc;
    if (num_agents > 1 && !pred_logits)
        return glue_fail(MZ_ERR_ARG, fn, "leaf policy logits required for later agents");
    if (int rc = glue_dtype(g, dtype)) return rc;
    glue_dispatch(dtype, g.A, [&](auto f16, auto tiles) {
        hipLaunchKernelGGL((k_joint_action_rows<decltype(f16)::value, decltype(tiles)::value>), dim3(g.B), dim3(kWave),
                           0, g.stream, pred_logits, num_agents, g.A, (const int *)row_agent, (const int *)factor,
                           factor_cols, (const int *)actions, (long long *)joint_out);
    });
    return glue_end(g);
}

int mz_policy_glue_later_rows(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int num_agents,
                              const int32_t *row_agent, double sampled_tau, float *probs_out, float *beta_out,
                              int32_t *later_out) {
    const char *fn = "mz_policy_glue_later_rows";
    Glue g;
    if (int rc = glue_begin(&g, fn, b, true)) return rc;
    if (int rc = rows_agents(g, num_agents, kMaxGridRows, row_agent)) return rc;
    if (!logits) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (!probs_out != !beta_out) return glue_fail(MZ_ERR_ARG, fn, "probs_out and beta_out go together");
    const int glue = probs_out ? 1 : 0, later = num_agents - 1;  // (a row of agent 0 has them all)
    if (later > 0 && !later_out) return glue_fail(MZ_ERR_ARG, fn, "later_out required for later agents");
    if (glue + later == 0) return glue_fail(MZ_ERR_ARG, fn, "no output asked for");
    if (int rc = glue_dtype(g, dtype)) return rc;
    if (row_stride < (int64_t)num_agents * g.A)
        return glue_fail(MZ_ERR_ARG, fn, "logits row does not hold every agent's actions");
    if (int rc = glue_tau(&g, sampled_tau, dtype == MZ_DT_F16)) return rc;  // as mz_policy_glue
    glue_dispatch(dtype, g.A, [&](auto f16, auto tiles) {
        hipLaunchKernelGGL((k_policy_glue_later_rows<decltype(f16)::value, decltype(tiles)::value>),
                           dim3(g.B, glue + later), dim3(kWave), 0, g.stream, logits, (long long)row_stride,
                           (const int *)row_agent, g.plan, num_agents, glue, g.use_pow, g.tau_inv, probs_out,
                           beta_out, (int *)later_out, g.hexp);
    });
    return glue_end(g);
}

int mz_joint_action_cached_rows(mz_batch *b, const int32_t *later_pool, int slots, const int32_t *idx_x,
                                int num_agents, const int32_t *row_agent, const int32_t *factor, int factor_cols,
                                const int32_t *actions, int64_t *joint_out) {
    const char *fn = "mz_joint_action_cached_rows";
    Glue g;
    if (int rc = glue_handle(&g, fn, b)) return rc;  // (any A: no row of actions is read)
    if (int rc = rows_agents(g, num_agents, kMaxGridRows, row_agent)) return rc;
    if (!actions || !joint_out) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (int rc = rows_factor(g, num_agents, factor, factor_cols)) return rc;
    if (num_agents > 1 && (!later_pool || !idx_x || slots < 1))
        return glue_fail(MZ_ERR_ARG, fn, "later-action pool and idx_x required for later agents");
    const long long n = (long long)g.B * num_agents;
    hipLaunchKernelGGL(k_joint_action_cached_rows, dim3((unsigned)((n + kCachedLanes - 1) / kCachedLanes)),
                       dim3(kCachedLanes), 0, g.stream, (const int *)later_pool, slots, (const int *)idx_x, g.B,
                       num_agents, (const int *)row_agent, (const int *)factor, factor_cols, (const int *)actions,
                       (long long *)joint_out);
    return glue_end(g);
}

// The joint glue: k_policy_glue / k_root_glue with an agent per grid row.  One lane per action for the
// _joint entry points (what mz_create's joint trees take); the _joint_wide ones take any A the handle
// has (`wide`, the trees of mz_create_wide_joint) with the same kernels' wider tile instantiations.
static int policy_glue_joint(const char *fn, bool wide, mz_batch *b, const void *logits, int dtype, int64_t row_stride,
                             int num_agents, double sampled_tau, float *probs_out, float *beta_out) {
    Glue g;
    if (int rc = glue_begin(&g, fn, b, wide)) return rc;
    if (num_agents < 1 || num_agents > kMaxGridRows) return glue_fail(MZ_ERR_ARG, fn, "bad agent count");
    if (!logits || !probs_out || !beta_out) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (int rc = glue_dtype(g, dtype)) return rc;
    if (row_stride < (int64_t)num_agents * g.A)
        return glue_fail(MZ_ERR_ARG, fn, "logits row does not hold every agent's actions");
    if (int rc = glue_tau(&g, sampled_tau, dtype == MZ_DT_F16)) return rc;  // as mz_policy_glue
    return launch_policy_glue(g, dtype, num_agents, logits, row_stride, 0, probs_out, beta_out);
}

static int root_glue_joint(const char *fn, bool wide, mz_batch *b, const void *logits, int dtype, int64_t row_stride,
                           int num_agents, const int32_t *legal, int64_t legal_stride, const float *noises,
                           double noise_eps, double sampled_tau, float *probs_out, float *beta_out,
                           float *noises_out) {
    Glue g;
    if (int rc = glue_begin(&g, fn, b, wide)) return rc;
    if (num_agents < 1 || num_agents > kMaxGridRows) return glue_fail(MZ_ERR_ARG, fn, "bad agent count");
    if (!logits || !noises || !probs_out || !beta_out || !noises_out) return glue_fail(MZ_ERR_ARG, fn, "null buffer");
    if (int rc = glue_dtype(g, dtype)) return rc;
    if (row_stride < (int64_t)num_agents * g.A)
        return glue_fail(MZ_ERR_ARG, fn, "logits row does not hold every agent's actions");
    if (legal && legal_stride < (int64_t)num_agents * g.A)
        return glue_fail(MZ_ERR_ARG, fn, "legal rows hold fewer than num_agents * A");
    if (int rc = glue_tau(&g, sampled_tau, false)) return rc;  // as mz_root_glue: beta is a float32 array
    return launch_root_glue(g, dtype, num_agents, logits, row_stride, 0, legal, legal_stride, noises, noise_eps,
                            probs_out, beta_out, noises_out);
}

int mz_policy_glue_joint(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int num_agents,
                         double sampled_tau, float *probs_out, float *beta_out) {
    return policy_glue_joint("mz_policy_glue_joint", false, b, logits, dtype, row_stride, num_agents, sampled_tau,
                             probs_out, beta_out);
}

int mz_policy_glue_joint_wide(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int num_agents,
                              double sampled_tau, float *probs_out, float *beta_out) {
    return policy_glue_joint("mz_policy_glue_joint_wide", true, b, logits, dtype, row_stride, num_agents, sampled_tau,
                             probs_out, beta_out);
}

int mz_root_glue_joint(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int num_agents,
                       const int32_t *legal, int64_t legal_stride, const float *noises, double noise_eps,
                       double sampled_tau, float *probs_out, float *beta_out, float *noises_out) {
    return root_glue_joint("mz_root_glue_joint", false, b, logits, dtype, row_stride, num_agents, legal, legal_stride,
                           noises, noise_eps, sampled_tau, probs_out, beta_out, noises_out);
}

int mz_root_glue_joint_wide(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int num_agents,
                            const int32_t *legal, int64_t legal_stride, const float *noises, double noise_eps,
                            double sampled_tau, float *probs_out, float *beta_out, float *noises_out) {
    return root_glue_joint("mz_root_glue_joint_wide", true, b, logits, dtype, row_stride, num_agents, legal,
                           legal_stride, noises, noise_eps, sampled_tau, probs_out, beta_out, noises_out);
}

int mz_policy_glue(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int64_t col_offset,
                   double sampled_tau, float *probs_out, float *beta_out) {
    return policy_glue("mz_policy_glue", false, b, logits, dtype, row_stride, col_offset, sampled_tau, probs_out,
                       beta_out);
}

int mz_policy_glue_wide(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int64_t col_offset,
                        double sampled_tau, float *probs_out, float *beta_out) {
    return policy_glue("mz_policy_glue_wide", true, b, logits, dtype, row_stride, col_offset, sampled_tau,
                       probs_out, beta_out);
}

int mz_root_glue(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int64_t col_offset,
                 const int32_t *legal, int64_t legal_stride, const float *noises, double noise_eps,
                 double sampled_tau, float *probs_out, float *beta_out, float *noises_out) {
    return root_glue("mz_root_glue", false, b, logits, dtype, row_stride, col_offset, legal, legal_stride, noises,
                     noise_eps, sampled_tau, probs_out, beta_out, noises_out);
}

int mz_root_glue_wide(mz_batch *b, const void *logits, int dtype, int64_t row_stride, int64_t col_offset,
                      const int32_t *legal, int64_t legal_stride, const float *noises, double noise_eps,
                      double sampled_tau, float *probs_out, float *beta_out, float *noises_out) {
    return root_glue("mz_root_glue_wide", true, b, logits, dtype, row_stride, col_offset, legal, legal_stride,
                     noises, noise_eps, sampled_tau, probs_out, beta_out, noises_out);
}

int mz_joint_action(mz_batch *b, const void *pred_logits, int dtype, int num_agents, int current_agent,
                    const int32_t *factor, int factor_cols, const int32_t *actions, int64_t *joint_out) {
    return joint_action("mz_joint_action", false, b, pred_logits, dtype, num_agents, current_agent, factor,
                        factor_cols, actions, joint_out);
}

int mz_joint_action_wide(mz_batch *b, const void *pred_logits, int dtype, int num_agents, int current_agent,
                         const int32_t *factor, int factor_cols, const int32_t *actions, int64_t *joint_out) {
    return joint_action("mz_joint_action_wide", true, b, pred_logits, dtype, num_agents, current_agent, factor,
                        factor_cols, actions, joint_out);
}

// mz_inverse_transform (wide false: supports past one wave are refused) and mz_inverse_transform_wide
static int inverse_transform(const char *fn, bool wide, mz_batch *b, void *stream, int stage, int n,
                             const void *value_in, int value_dtype, int64_t value_stride, int value_lo, int value_hi,
                             const void *reward_in, int reward_dtype, int64_t reward_stride, int reward_lo,
                             int reward_hi, float *value_out, float *reward_out) {
    hipStream_t s = (hipStream_t)stream;
    if (b) {  // the handle's device current, its stream
        int B = 0, A = 0;
        int rc = mz_internal_launch_info(b, &B, &A, &s);
        if (rc) return rc;
    }
    if (stage != MZ_INV_LOGITS && stage != MZ_INV_PROBS && stage != MZ_INV_EXPECTATION)
        return glue_fail(MZ_ERR_ARG, fn, "bad stage");
    if (n < 0) return glue_fail(MZ_ERR_ARG, fn, "n must be >= 0");
    InvHead heads[2] = {}, wheads[2] = {};  // heads of up to 64 support elements (or scalars); longer ones
    InvPlan wplans[2] = {};
    int nh = 0, nw = 0, wide_it = 0;
    const struct {
        const void *in;
        int dtype;
        int64_t stride;
        int lo, hi;
        float *out;
    } args[2] = {{value_in, value_dtype, value_stride, value_lo, value_hi, value_out},
                 {reward_in, reward_dtype, reward_stride, reward_lo, reward_hi, reward_out}};
    for (const auto &a : args) {
        if (!a.in && !a.out) continue;  // this head is not asked for
        if (!a.in || !a.out) return glue_fail(MZ_ERR_ARG, fn, "a head needs both its input and its output");
        if (a.dtype != MZ_DT_F32 && !(a.dtype == MZ_DT_F16 && stage == MZ_INV_LOGITS))
            return glue_fail(MZ_ERR_ARG, fn, "bad dtype (logits: f32 or f16; probabilities and expectations: f32)");
        if (a.hi < a.lo) return glue_fail(MZ_ERR_ARG, fn, "support hi < lo");
        const int64_t S = (int64_t)a.hi - a.lo + 1;
        if (stage != MZ_INV_EXPECTATION) {
            if (S > kWave && !wide)
                return glue_fail(MZ_ERR_UNSUPPORTED, fn, "support size > 64 (one lane per support element)");
            if (S > kInvWideMax)
                return glue_fail(MZ_ERR_UNSUPPORTED, fn, "support size > 1024 (torch's softmax changes kernel there)");
            if (a.stride < S) return glue_fail(MZ_ERR_ARG, fn, "row stride below the support size");
            if (S > kWave) {  // k_inverse_rows_wide, with the plan of torch's sum for this S and n
                InvPlan plan{};
                inverse_sum_plan((int)S, n > 0 ? n : 1, &plan.vec, &plan.bw);
                plan.nit = 2;
                while (plan.nit * kWave < S) plan.nit <<= 1;
                if (plan.nit > wide_it) wide_it = plan.nit;
                wplans[nw] = plan;
                wheads[nw++] = InvHead{a.in, a.out, (long long)a.stride, a.lo, (int)S, a.dtype == MZ_DT_F16};
                continue;
            }
        } else if (a.stride < 1) {
            return glue_fail(MZ_ERR_ARG, fn, "row stride must be >= 1");
        }
        heads[nh++] = InvHead{a.in, a.out, (long long)a.stride, a.lo, (int)(S > kWave ? 0 : S), a.dtype == MZ_DT_F16};
    }
    if (nh + nw == 0) return glue_fail(MZ_ERR_ARG, fn, "both heads are null");
    if (n == 0) return MZ_OK;
    if (nw) {
        const long long blocks = ((long long)n + kInvWaves - 1) / kInvWaves;
        const dim3 grid((unsigned)(blocks < kInvMaxGrid ? blocks : kInvMaxGrid), nw);
        const int probs = stage == MZ_INV_PROBS ? 1 : 0;
#define MZ_INV_WIDE_LAUNCH(IT)                                                                              \
    hipLaunchKernelGGL(k_inverse_rows_wide<IT>, grid, dim3(kInvLanes), 0, s, wheads[0], wheads[1], wplans[0], \
                       wplans[1], n, probs)
        if (wide_it == 2)
            MZ_INV_WIDE_LAUNCH(2);
        else if (wide_it == 4)
            MZ_INV_WIDE_LAUNCH(4);
        else if (wide_it == 8)
            MZ_INV_WIDE_LAUNCH(8);
        else
            MZ_INV_WIDE_LAUNCH(16);
#undef MZ_INV_WIDE_LAUNCH
    }
    if (nh && stage == MZ_INV_EXPECTATION) {
        const long long blocks = ((long long)n + kInvLanes - 1) / kInvLanes;
        hipLaunchKernelGGL(k_inverse_scalars, dim3((unsigned)(blocks < kInvMaxGrid ? blocks : kInvMaxGrid), nh),
                           dim3(kInvLanes), 0, s, heads[0], heads[1], n);
    } else if (nh) {  // (0: every head went to the wide kernel)
        const long long blocks = ((long long)n + kInvWaves - 1) / kInvWaves;
        hipLaunchKernelGGL(k_inverse_rows, dim3((unsigned)(blocks < kInvMaxGrid ? blocks : kInvMaxGrid), nh),
                           dim3(kInvLanes), 0, s, heads[0], heads[1], n, stage == MZ_INV_PROBS ? 1 : 0);
    }
    if (b) mz_internal_enqueued(b);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mz_internal_fail(MZ_ERR_DEVICE, hipGetErrorString(e));
    return MZ_OK;
}

int mz_inverse_transform(mz_batch *b, void *stream, int stage, int n, const void *value_in, int value_dtype,
                         int64_t value_stride, int value_lo, int value_hi, const void *reward_in, int reward_dtype,
                         int64_t reward_stride, int reward_lo, int reward_hi, float *value_out, float *reward_out) {
    return inverse_transform("mz_inverse_transform", false, b, stream, stage, n, value_in, value_dtype, value_stride,
                             value_lo, value_hi, reward_in, reward_dtype, reward_stride, reward_lo, reward_hi, value_out,
                             reward_out);
}

int mz_inverse_transform_wide(mz_batch *b, void *stream, int stage, int n, const void *value_in, int value_dtype,
                              int64_t value_stride, int value_lo, int value_hi, const void *reward_in,
                              int reward_dtype, int64_t reward_stride, int reward_lo, int reward_hi, float *value_out,
                              float *reward_out) {
    return inverse_transform("mz_inverse_transform_wide", true, b, stream, stage, n, value_in, value_dtype,
                             value_stride, value_lo, value_hi, reward_in, reward_dtype, reward_stride, reward_lo,
                             reward_hi, value_out, reward_out);
}

int mz_inverse_sum_plan(int S, int n, int *vectorized, int *block_width) {
    if (!vectorized || !block_width) return mz_internal_fail(MZ_ERR_ARG, "mz_inverse_sum_plan: null argument");
    if (S < 1 || n < 1) return mz_internal_fail(MZ_ERR_ARG, "mz_inverse_sum_plan: S and n must be >= 1");
    if (S > kInvWideMax) return mz_internal_fail(MZ_ERR_UNSUPPORTED, "mz_inverse_sum_plan: S > 1024");
    inverse_sum_plan(S, n, vectorized, block_width);
    return MZ_OK;
}

int mz_wide_sum_plan(int n, int32_t *starts, int32_t *lens, int32_t *num_blocks) {
    if (!starts || !lens || !num_blocks) return mz_internal_fail(MZ_ERR_ARG, "mz_wide_sum_plan: null argument");
    if (n < 1 || n > kWideMax) return mz_internal_fail(MZ_ERR_UNSUPPORTED, "mz_wide_sum_plan: n outside 1..255");
    const unsigned plan = sum_plan(n);
    int k = 0;
    for (int i = 0, start = 0; i < kMaxBlocks; ++i) {
        lens[i] = (int32_t)(plan >> (8 * i) & 0xffu);
        starts[i] = lens[i] ? start : 0;
        start += lens[i];
        if (lens[i]) ++k;
    }
    *num_blocks = k;
    return MZ_OK;
}

// nodes and memset nodes of a graph, child graphs (hipGraphNodeTypeGraph: a nested capture, an
// embedded graph) included
static hipError_t census(hipGraph_t g, int depth, int *total, int *memsets) {
    if (depth > 16) return hipErrorInvalidValue;
    size_t n = 0;
    hipError_t e = hipGraphGetNodes(g, nullptr, &n);
    if (e != hipSuccess) return e;
    hipGraphNode_t *nodes = (hipGraphNode_t *)malloc(sizeof(hipGraphNode_t) * (n ? n : 1));
    if (!nodes) return hipErrorOutOfMemory;
    e = hipGraphGetNodes(g, nodes, &n);
    *total += (int)n;
    for (size_t k = 0; e == hipSuccess && k < n; ++k) {
        hipGraphNodeType ty;
        e = hipGraphNodeGetType(nodes[k], &ty);
        if (e != hipSuccess) break;
        if (ty == hipGraphNodeTypeMemset) {
            ++*memsets;
        } else if (ty == hipGraphNodeTypeGraph) {
            hipGraph_t child = nullptr;
            e = hipGraphChildGraphNodeGetGraph(nodes[k], &child);
            if (e == hipSuccess) e = census(child, depth + 1, total, memsets);
        }
    }
    free(nodes);
    return e;
}

int mz_graph_census(void *graph, int *total_nodes, int *memset_nodes) {
    if (!graph || !total_nodes || !memset_nodes) return mz_internal_fail(MZ_ERR_ARG, "mz_graph_census: null argument");
    int total = 0, ms = 0;
    hipError_t e = census((hipGraph_t)graph, 0, &total, &ms);
    if (e != hipSuccess) return mz_internal_fail(MZ_ERR_DEVICE, hipGetErrorString(e));
    *total_nodes = total;
    *memset_nodes = ms;
    return MZ_OK;
}

}  // extern "C"
