// mzconsume.hip — on-device consumers of the search output (include/mzconsume.h).
//
// The reference workers make their per-root decisions in Python after each search:
//   select_action + eps_greedy_action (core/utils.py:289-334, called at selfplay_worker.py:228-252),
//   the stored policy probability and visit entropy (selfplay_worker.py:278-293),
//   the reanalyze action and policy product (reanalyze_worker.py:296-332).
//   the reanalyze batch's value / reward targets (reanalyze_worker.py:137-157, :186-204) and the
//   advantage normalisation of make_batch (:466-473).
// Here one lane handles one root and walks its row sequentially, in the reference's own order of
// floating-point operations (Python's left-to-right sum, numpy's sequential cumsum, IEEE
// division), so every probability and index is bit-identical.  The work is a few hundred bytes per
// root, far below any bandwidth bound: these kernels exist to keep the search output on the device
// (no device-to-host copy of the per-root lists between the search and the environment step).
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mzconsume.h"
#include "mz_internal.h"

namespace {

constexpr int kLanes = 64;

constexpr int kPowTableMax = MZ_SELECT_POW_TABLE_MAX;  // the host's table holds v ** e for v in 0..kPowTableMax

// How v ** e is computed for a visit count v (core/utils.py:302: Python's float power of an int, the
// host libm's pow).  ipow > 0: the repeated product x * x * .. (ipow factors) for v <= exact_max, the
// largest v with v ** ipow <= 2**53: every partial product is then an integer below 2**53, so the
// product is exact and equal to pow.  table: the host's own pow((double)v, e) for v in 0..kPowTableMax
// (NULL: none), for every count the product does not cover.  A count that neither covers refuses its row.
struct PowPlan {
    int ipow, exact_max;
    const double *table;
};

__device__ __forceinline__ bool pow_in_product(int v, const PowPlan &p) { return p.ipow > 0 && v <= p.exact_max; }

__device__ __forceinline__ bool pow_covered(int v, const PowPlan &p) {
    return pow_in_product(v, p) || (p.table && v >= 0 && v <= kPowTableMax);
}

// v ** e for a covered count (pow_covered)
__device__ __forceinline__ double visit_pow(int v, const PowPlan &p) {
    if (pow_in_product(v, p)) {
        const double x = (double)v;
        double r = x;
        for (int k = 1; k < p.ipow; ++k) r *= x;
        return r;
    }
    return p.table[v];
}

// select_action for root i (core/utils.py:289-316): the chosen child's position, written to pos_out
// with the entropy; -1 (and a NaN entropy) for a root without children or visits, of a degree past the
// row's width, or holding a count whose power is not covered (PowPlan).  The body of k_select_actions
// and of k_select_actions_joint, which differ in the action columns they copy.
__device__ __forceinline__ int select_position(int i, const int *__restrict__ deg, const int *__restrict__ visits,
                                               int width, const PowPlan &pp, int deterministic,
                                               const double *__restrict__ uniforms, int *pos_out, double *ent_out) {
    const int n = deg[i];
    const int *row = visits + (long long)i * width;
    long long vsum = 0;
    bool covered = true;
    if (n <= width)  // (a degree past the row's width is refused below, and never read)
        for (int j = 0; j < n; ++j) {
            vsum += row[j];
            covered = covered && pow_covered(row[j], pp);
        }
    if (n <= 0 || n > width || vsum <= 0 || !covered) {  // assert sum(visit_counts) > 0 (core/utils.py:301)
        pos_out[i] = -1;
        if (ent_out) ent_out[i] = NAN;
        return -1;
    }
    // total_count = sum(action_probs): Python's sum, left to right from 0 (utils.py:304)
    double total = 0.0;
    for (int j = 0; j < n; ++j) total += visit_pow(row[j], pp);
    if (!(total < INFINITY)) {  // the powers overflow: numpy's choice refuses the NaN probabilities
        pos_out[i] = -1;
        if (ent_out) ent_out[i] = NAN;
        return -1;
    }
    int pos = 0;
    if (deterministic) {
        for (int j = 1; j < n; ++j)
            if (row[j] > row[pos]) pos = j;  // np.argmax: first maximum
    } else {
        // np_random.choice(n, p=probs): cdf = probs.cumsum(); cdf /= cdf[-1];
        // cdf.searchsorted(u, side='right')
        double last = 0.0;
        for (int j = 0; j < n; ++j) last += visit_pow(row[j], pp) / total;
        const double u = uniforms[i];
        double c = 0.0;
        pos = n - 1;
        for (int j = 0; j < n; ++j) {
            c += visit_pow(row[j], pp) / total;
            if (c / last > u) {
                pos = j;
                break;
            }
        }
    }
    pos_out[i] = pos;
    if (ent_out) {
        // scipy.stats.entropy(action_probs, base=2): pk / sum(pk), sum of -pk log pk, / log(2)
        double ps = 0.0;
        for (int j = 0; j < n; ++j) ps += visit_pow(row[j], pp) / total;
        double h = 0.0;
        for (int j = 0; j < n; ++j) {
            const double pk = (visit_pow(row[j], pp) / total) / ps;
            if (pk > 0.0) h -= pk * log(pk);
        }
        ent_out[i] = h / log(2.0);
    }
    return pos;
}

__global__ __launch_bounds__(kLanes) void k_select_actions(int B, int N, const int *__restrict__ deg,
                                                           const int *__restrict__ visits,
                                                           const int *__restrict__ actions, int width, PowPlan pp,
                                                           int deterministic,
                                                           const double *__restrict__ uniforms, int *pos_out,
                                                           int *act_out, double *ent_out) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= B) return;
    const int pos = select_position(i, deg, visits, width, pp, deterministic, uniforms, pos_out, ent_out);
    // sampled_actions[pos, 0]
    act_out[i] = pos < 0 ? -1 : actions[(long long)i * width * N + (long long)pos * N];
}

// mz_select_actions_joint: the chosen child's whole joint action, sampled_actions[pos] (core/test.py:
// 101-107), into row i of act_out [B, N]
__global__ __launch_bounds__(kLanes) void k_select_actions_joint(int B, int N, const int *__restrict__ deg,
                                                                 const int *__restrict__ visits,
                                                                 const int *__restrict__ actions, int width,
                                                                 PowPlan pp, int deterministic,
                                                                 const double *__restrict__ uniforms, int *pos_out,
                                                                 int *act_out, double *ent_out) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= B) return;
    const int pos = select_position(i, deg, visits, width, pp, deterministic, uniforms, pos_out, ent_out);
    for (int k = 0; k < N; ++k)
        act_out[(long long)i * N + k] = pos < 0 ? -1 : actions[((long long)i * width + pos) * N + k];
}

__global__ __launch_bounds__(kLanes) void k_eps_greedy(int B, int A, const int *__restrict__ legal, long long stride,
                                                       float eps, const float *__restrict__ u_eps,
                                                       const double *__restrict__ u_cat, int *action_io) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= B) return;
    if (!(u_eps[i] < eps)) return;  // pick_random = (rand < eps) in float32 (utils.py:327-328)
    const int *w = legal + (long long)i * stride;
    long long tot = 0;
    for (int a = 0; a < A; ++a) tot += w[a];
    if (tot <= 0) return;
    // Categorical(legal_action_mask).sample() (utils.py:329): inverse cdf of the mask weights
    const double u = u_cat[i];
    long long c = 0;
    for (int a = 0; a < A; ++a) {
        c += w[a];
        if ((double)c / (double)tot > u) {
            action_io[i] = a;
            return;
        }
    }
}

__global__ __launch_bounds__(kLanes) void k_marginal_policy(int B, int A, const int *__restrict__ marginal,
                                                            long long mstride, const int *__restrict__ legal,
                                                            long long lstride, int mode, int *action_io,
                                                            double *prob_io, double *ent_out) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= B) return;
    const int *m = marginal + (long long)i * mstride;
    long long msum = 0;
    for (int a = 0; a < A; ++a) msum += m[a];
    if (mode == MZ_MARGINAL_ARGMAX) {
        if (msum <= 0) {  // the reference draws np_random.choice(legal_indices) (reanalyze_worker.py:313-315)
            action_io[i] = -1;
            return;
        }
        // np.argmax(marginal_visits * legal_actions): first maximum of the int64 products
        const int *l = legal + (long long)i * lstride;
        int best = 0;
        long long bv = (long long)m[0] * l[0];
        for (int a = 1; a < A; ++a) {
            const long long v = (long long)m[a] * l[a];
            if (v > bv) bv = v, best = a;
        }
        action_io[i] = best;
    }
    const int act = action_io[i];
    if (msum <= 0) {  // selfplay_worker.py:287-288
        prob_io[i] *= 1.0 / (double)A;
        if (ent_out) ent_out[i] = 0.0;
        return;
    }
    const double s = (double)msum;
    // prob *= (marginal / np.sum(marginal))[action]  (selfplay_worker.py:284-286, reanalyze_worker.py:336-343)
    prob_io[i] *= (act >= 0 && act < A) ? (double)m[act] / s : NAN;
    if (ent_out) {
        double h = 0.0;  // -np.sum(p * np.log(p + 1e-9))  (selfplay_worker.py:286)
        for (int a = 0; a < A; ++a) {
            const double p = (double)m[a] / s;
            h += p * log(p + 1e-9);
        }
        ent_out[i] = -h;
    }
}

// MZ_MARGINAL_ARGMAX_LEGAL: the action of one agent turn of the full-game reanalysis
// (reanalyze_worker.py:563-570).  Writes action_io only.
__global__ __launch_bounds__(kLanes) void k_marginal_argmax_legal(int B, int A, const int *__restrict__ marginal,
                                                                  long long mstride, const int *__restrict__ legal,
                                                                  long long lstride, int *action_io) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= B) return;
    const int *m = marginal + (long long)i * mstride;
    const int *l = legal + (long long)i * lstride;
    // masked_visits = marginal_visits * legal_actions; np.sum(masked_visits) > 0, else the host draws
    int best = 0;
    long long bv = (long long)m[0] * l[0], sum = bv;
    for (int a = 1; a < A; ++a) {
        const long long v = (long long)m[a] * l[a];
        sum += v;
        if (v > bv) bv = v, best = a;  // np.argmax: first maximum
    }
    action_io[i] = sum > 0 ? best : -1;
}

// ---- reanalyze batch targets (reanalyze_worker.py:376-489) -----------------------------------

// One row of _prepare_reward_value_re (:137-157) / _prepare_reward_value_non_re (:186-204).  The
// reward term and the accumulator follow numpy 2 scalar promotion (include/mzconsume.h); the
// translation unit is built with -ffp-contract=off, so `acc += r * d` stays a product and a sum.
template <typename R, typename S>
__global__ __launch_bounds__(kLanes) void k_value_targets(
    int mode, long long row0, int n, int G, int U1, const float *__restrict__ value,
    const double *__restrict__ td_pow, const int *__restrict__ td, const int *__restrict__ pos,
    const int *__restrict__ traj_len, const int *__restrict__ reward_len, const R *__restrict__ rewards,
    const S *__restrict__ stored, long long L, const double *__restrict__ dpow, const float *__restrict__ dpow32,
    int td_max, double *__restrict__ out_value, double *__restrict__ out_reward) {
    const int t = blockIdx.x * kLanes + threadIdx.x;
    if (t >= n) return;
    const long long j = row0 + t;
    const long long g = j / U1;
    const int k = (int)(j % U1);
    double v = 0.0, rew = 0.0;
    if (g < G && pos[g] >= 0) {
        const long long rl = min((long long)reward_len[g], L);  // (clamped: rows hold L entries)
        const long long tl = min((long long)traj_len[g], rl);
        const long long cur = (long long)pos[g] + k;
        if (cur < tl) {  // else target_values.append(0.0), target_rewards.append(0.0)
            const int tdg = max(0, min(td[g], td_max));
            const long long boot = cur + tdg;                // bootstrap_index
            const int cnt = (int)(min(boot, rl) - cur);       // len(reward_lst[current_index:bootstrap_index])
            const R *r = rewards + g * L + cur;
            rew = (double)r[0];
            constexpr bool r32 = sizeof(R) == 4;
            if (mode == MZ_VALUE_RE) {
                v = (double)value[t] * td_pow[t];               // :138
                v = v * (boot < tl ? 1.0 : 0.0);                // :139
                for (int i = 0; i < cnt; ++i) {
                    if constexpr (r32) v += (double)((float)r[i] * dpow32[i]);
                    else v += (double)r[i] * dpow[i];
                }
            } else {
                const bool has = boot < tl;  // else bootstrap_value = 0, a Python int
                if (r32 && (sizeof(S) == 4 || !has)) {
                    float a = has ? (float)stored[g * L + boot] : 0.0f;
                    for (int i = 0; i < cnt; ++i) a += (float)r[i] * dpow32[i];
                    v = (double)a;
                } else {
                    v = has ? (double)stored[g * L + boot] : 0.0;
                    for (int i = 0; i < cnt; ++i) {
                        if constexpr (r32) v += (double)((float)r[i] * dpow32[i]);
                        else v += (double)r[i] * dpow[i];
                    }
                }
            }
        }
    }
    out_value[t] = v;
    out_reward[t] = rew;
}

// numpy's pairwise sum as a plan (include/mzconsume.h mz_pairwise_plan).
constexpr int kAdvThreads = 1024;
constexpr int kAdvMaxN = 65536;
constexpr int kPlanMaxLeaves = 1024;  // a leaf of a split sum holds at least 64 elements
constexpr int kPlanMaxDepth = 32;     // operand stack of the postfix joins (LDS)
constexpr int kPairwiseBlock = 128;   // numpy's PW_BLOCKSIZE
constexpr int kReduceChunk = 8192;    // numpy's default buffer size, in elements

struct PairwisePlan {
    std::vector<int32_t> starts, ops;
    int depth = 0;
};

void pairwise_rec(int start, int n, PairwisePlan &p) {
    if (n <= kPairwiseBlock) {
        p.starts.push_back(start);
        p.ops.push_back(0);
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    pairwise_rec(start, n2, p);
    pairwise_rec(start + n2, n - n2, p);
    p.ops.push_back(1);
}

bool pairwise_plan(int n, PairwisePlan &p) {
    if (n < 1 || n > kAdvMaxN) return false;
    // np.add.reduce hands its inner loop at most one buffer (numpy's default bufsize, 8192
    // elements) at a time: the chunks are summed pairwise and accumulated in order
    for (int start = 0; start < n; start += kReduceChunk) {
        pairwise_rec(start, std::min(kReduceChunk, n - start), p);
        if (start) p.ops.push_back(1);
    }
    p.starts.push_back(n);
    int sp = 0;
    for (int32_t o : p.ops) {
        sp += o ? -1 : 1;
        p.depth = std::max(p.depth, sp);
    }
    return sp == 1 && p.depth <= kPlanMaxDepth && (int)p.starts.size() - 1 <= kPlanMaxLeaves;
}

// element j of the summed array: pass 0 where(valid, adv, 0), pass 1 where(valid, (adv - mean)^2, 0)
template <int PASS>
__device__ __forceinline__ double adv_elem(const float *q, const float *pred, const unsigned char *mask, int j,
                                           double mean) {
    const double a = (double)q[j] - (double)pred[j];
    const bool valid = mask[j] && a == a;  // nanmean / nanstd skip every NaN
    if (PASS == 0) return valid ? a : 0.0;
    const double d = a - mean;
    return valid ? d * d : 0.0;
}

// One pairwise sum by the whole workgroup: lanes 8b + i run accumulator i of leaf b (128 leaves a
// round), lane 8b combines leaf b, then lane 0 joins the leaf sums in recursion order.
template <int PASS>
__device__ double pairwise_pass(const float *q, const float *pred, const unsigned char *mask, const int *starts,
                                const int *ops, int nl, int nops, double mean, double *acc, double *leaf,
                                double *stack, double *result) {
    const int tid = threadIdx.x, i = tid & 7;
    for (int base = 0; base < nl; base += kAdvThreads / 8) {
        const int b = base + (tid >> 3);
        int s = 0, len = 0;
        if (b < nl) {
            s = starts[b];
            len = starts[b + 1] - s;
        }
        const int body = len - (len & 7);
        if (len >= 8) {
            double r = adv_elem<PASS>(q, pred, mask, s + i, mean);
            for (int k = 8 + i; k < body; k += 8) r += adv_elem<PASS>(q, pred, mask, s + k, mean);
            acc[tid] = r;
        }
        __syncthreads();
        if (b < nl && i == 0) {
            double res;
            if (len < 8) {
                res = 0.0;
                for (int k = 0; k < len; ++k) res += adv_elem<PASS>(q, pred, mask, s + k, mean);
            } else {
                const double *r = acc + tid;
                res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
                for (int k = body; k < len; ++k) res += adv_elem<PASS>(q, pred, mask, s + k, mean);
            }
            leaf[b] = res;
        }
        __syncthreads();
    }
    if (tid == 0) {
        int sp = 0, nb = 0;
        for (int o = 0; o < nops; ++o) {
            if (ops[o] == 0) {
                stack[sp++] = leaf[nb++];
            } else {
                --sp;
                stack[sp - 1] = stack[sp - 1] + stack[sp];
            }
        }
        *result = 0.0 + stack[0];  // np.add.reduce starts from the identity
    }
    __syncthreads();
    const double out = *result;
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(kAdvThreads) void k_normalize_advantage(
    int n, const float *__restrict__ q, const float *__restrict__ pred, const unsigned char *__restrict__ mask,
    const int *__restrict__ starts, const int *__restrict__ ops, int nl, int nops, double *__restrict__ adv_out,
    double *__restrict__ stats_out) {
    __shared__ double acc[kAdvThreads];
    __shared__ double leaf[kPlanMaxLeaves];
    __shared__ double stack[kPlanMaxDepth];
    __shared__ double result;
    __shared__ int cnt_s;
    const int tid = threadIdx.x;
    if (tid == 0) cnt_s = 0;
    __syncthreads();
    int c = 0;
    for (int j = tid; j < n; j += kAdvThreads) {
        const double a = (double)q[j] - (double)pred[j];
        c += (mask[j] && a == a) ? 1 : 0;
    }
    if (c) atomicAdd(&cnt_s, c);
    __syncthreads();
    const double cnt = (double)cnt_s;
    const double tot = pairwise_pass<0>(q, pred, mask, starts, ops, nl, nops, 0.0, acc, leaf, stack, &result);
    const double mean = tot / cnt;  // 0 / 0 = NaN when nothing is valid, as np.nanmean
    const double sq = pairwise_pass<1>(q, pred, mask, starts, ops, nl, nops, mean, acc, leaf, stack, &result);
    const double sd = sqrt(sq / cnt);
    if (tid == 0) {
        stats_out[0] = mean;
        stats_out[1] = sd;
    }
    const double den = sd + 1e-5;
    for (int j = tid; j < n; j += kAdvThreads) {
        const double a = (double)q[j] - (double)pred[j];
        adv_out[j] = mask[j] ? (a - mean) / den : 0.0;  // batch_sampled_adv[~masks] = 0.
    }
}

// The device copy of each n's plan: [starts (nl + 1) | ops (nops)], built on first use and kept.
struct DevicePlan {
    int device, n, nl, nops;
    int32_t *buf;
};
std::mutex g_plan_lock;
std::vector<DevicePlan> g_plans;
constexpr size_t kMaxPlans = 64;

int device_plan(int n, hipStream_t stream, DevicePlan *out) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return mz_internal_fail(MZ_ERR_DEVICE, "mz_normalize_advantage: no device");
    std::lock_guard<std::mutex> guard(g_plan_lock);
    for (const DevicePlan &p : g_plans)
        if (p.device == device && p.n == n) {
            *out = p;
            return MZ_OK;
        }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return mz_internal_fail(MZ_ERR_RUNTIME,
                                "mz_normalize_advantage: first call for this n inside a stream capture "
                                "(the plan is uploaded on first use: call once before capturing)");
    }
    PairwisePlan plan;
    if (!pairwise_plan(n, plan)) return mz_internal_fail(MZ_ERR_UNSUPPORTED, "mz_normalize_advantage: n outside 1..65536");
    DevicePlan d{device, n, (int)plan.starts.size() - 1, (int)plan.ops.size(), nullptr};
    std::vector<int32_t> host(plan.starts);
    host.insert(host.end(), plan.ops.begin(), plan.ops.end());
    if (g_plans.size() >= kMaxPlans) {  // (hipFree waits for the device: no launch still reads it)
        (void)hipFree(g_plans.front().buf);
        g_plans.erase(g_plans.begin());
    }
    if (hipMalloc((void **)&d.buf, host.size() * sizeof(int32_t)) != hipSuccess ||
        hipMemcpy(d.buf, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
        if (d.buf) (void)hipFree(d.buf);
        (void)hipGetLastError();
        return mz_internal_fail(MZ_ERR_DEVICE, "mz_normalize_advantage: plan upload failed");
    }
    g_plans.push_back(d);
    *out = d;
    return MZ_OK;
}

// The host half of PowPlan for e = 1 / temperature: the product's exponent and domain, from e alone.
// needs_table: some count in 0..kPowTableMax lies outside the product's domain.
struct HostPowPlan {
    double e;
    int ipow, exact_max;
    bool needs_table;
};

HostPowPlan host_pow_plan(double temperature) {
    HostPowPlan p{1.0 / temperature, 0, -1, true};  // 1 / temperature, as Python computes it
    if (p.e == floor(p.e) && p.e >= 1.0 && p.e <= 8.0) {
        p.ipow = (int)p.e;
        // the largest int32 v with v ** ipow <= 2**53, in exact integer arithmetic
        const unsigned __int128 lim = (unsigned __int128)1 << 53;
        long long lo = 1, hi = 0x7fffffffLL;
        while (lo < hi) {
            const long long mid = (lo + hi + 1) / 2;
            unsigned __int128 r = 1;
            for (int k = 0; k < p.ipow && r <= lim; ++k) r *= (unsigned __int128)mid;  // (r < 2**84: no overflow)
            if (r <= lim) lo = mid;
            else hi = mid - 1;
        }
        p.exact_max = (int)lo;
        p.needs_table = p.exact_max < kPowTableMax;
    }
    return p;
}

// table[v] = v ** e as the reference's Python computes it: the host libm's pow of float(v)
void fill_pow_table(double e, double *table, int len) {
    for (int v = 0; v < len; ++v) table[v] = pow((double)v, e);
}

// The device copy of each exponent's table, built on first use and kept (as the pairwise plans).
struct DevicePowTable {
    int device;
    double e;
    double *buf;
};
std::mutex g_pow_lock;
std::vector<DevicePowTable> g_pow_tables;
constexpr size_t kMaxPowTables = 16;

int device_pow_table(const std::string &name, double e, hipStream_t stream, const double **out) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return mz_internal_fail(MZ_ERR_DEVICE, (name + ": no device").c_str());
    std::lock_guard<std::mutex> guard(g_pow_lock);
    for (const DevicePowTable &t : g_pow_tables)
        if (t.device == device && t.e == e) {
            *out = t.buf;
            return MZ_OK;
        }
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return mz_internal_fail(MZ_ERR_RUNTIME,
                                (name + ": first call for this temperature inside a stream capture (its power "
                                        "table is uploaded on first use: call once before capturing)").c_str());
    }
    std::vector<double> host(kPowTableMax + 1);
    fill_pow_table(e, host.data(), (int)host.size());
    if (g_pow_tables.size() >= kMaxPowTables) {  // (hipFree waits for the device: no launch still reads it)
        (void)hipFree(g_pow_tables.front().buf);
        g_pow_tables.erase(g_pow_tables.begin());
    }
    DevicePowTable d{device, e, nullptr};
    if (hipMalloc((void **)&d.buf, host.size() * sizeof(double)) != hipSuccess ||
        hipMemcpy(d.buf, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        if (d.buf) (void)hipFree(d.buf);
        (void)hipGetLastError();
        return mz_internal_fail(MZ_ERR_DEVICE, (name + ": power table upload failed").c_str());
    }
    g_pow_tables.push_back(d);
    *out = d.buf;
    return MZ_OK;
}

// mz_internal_launch_info with the handle's active roots for B: the consumers' buffers hold rows
// [0, active) (include/mzdriver.h mz_set_active_roots)
int consumer_info(mz_batch *b, int *B, int *A, hipStream_t *stream) {
    int rc = mz_internal_launch_info(b, B, A, stream);
    if (rc) return rc;
    *B = mz_internal_active_roots(b);
    return MZ_OK;
}

// the stream of the handle (b != NULL) or the caller's (include/mzconsume.h)
int target_stream(mz_batch *b, void *stream, hipStream_t *out) {
    if (!b) {
        *out = (hipStream_t)stream;
        return MZ_OK;
    }
    int B = 0, A = 0;
    return mz_internal_launch_info(b, &B, &A, out);
}

int launch_status() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return mz_internal_fail(MZ_ERR_DEVICE, hipGetErrorString(e));
    return MZ_OK;
}

}  // namespace

extern "C" {

// mz_select_actions (joint false: agent 0's action, [B]) and mz_select_actions_joint ([B, N])
static int select_actions(const char *fn, bool joint, mz_batch *b, const int32_t *degrees, const int32_t *visits,
                          const int32_t *actions, int width, double temperature, int deterministic,
                          const double *uniforms, int32_t *pos_out, int32_t *action_out, double *entropy_out) {
    int B = 0, A = 0;
    hipStream_t stream = nullptr;
    int rc = consumer_info(b, &B, &A, &stream);
    if (rc) return rc;
    const std::string name(fn);
    if (!degrees || !visits || !actions || !pos_out || !action_out || (!deterministic && !uniforms))
        return mz_internal_fail(MZ_ERR_ARG, (name + ": null buffer").c_str());
    if (width < 1) return mz_internal_fail(MZ_ERR_ARG, (name + ": width must be >= 1").c_str());
    if (!(temperature > 0.0)) return mz_internal_fail(MZ_ERR_ARG, (name + ": temperature must be > 0").c_str());
    const HostPowPlan hp = host_pow_plan(temperature);
    PowPlan pp{hp.ipow, hp.exact_max, nullptr};
    if (hp.needs_table) {
        rc = device_pow_table(name, hp.e, stream, &pp.table);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(joint ? k_select_actions_joint : k_select_actions, dim3((B + kLanes - 1) / kLanes),
                       dim3(kLanes), 0, stream, B, mz_internal_agent_num(b), (const int *)degrees,
                       (const int *)visits, (const int *)actions, width, pp, deterministic, uniforms,
                       (int *)pos_out, (int *)action_out, entropy_out);
    mz_internal_enqueued(b);
    return launch_status();
}

int mz_select_actions(mz_batch *b, const int32_t *degrees, const int32_t *visits, const int32_t *actions, int width,
                      double temperature, int deterministic, const double *uniforms, int32_t *pos_out,
                      int32_t *action_out, double *entropy_out) {
    return select_actions("mz_select_actions", false, b, degrees, visits, actions, width, temperature, deterministic,
                          uniforms, pos_out, action_out, entropy_out);
}

int mz_select_actions_joint(mz_batch *b, const int32_t *degrees, const int32_t *visits, const int32_t *actions,
                            int width, double temperature, int deterministic, const double *uniforms,
                            int32_t *pos_out, int32_t *action_out, double *entropy_out) {
    return select_actions("mz_select_actions_joint", true, b, degrees, visits, actions, width, temperature,
                          deterministic, uniforms, pos_out, action_out, entropy_out);
}

int mz_select_pow_plan(double temperature, int32_t *ipow, int32_t *exact_max, int32_t *uses_table, double *table,
                       int table_len) {
    if (!ipow || !exact_max || !uses_table) return mz_internal_fail(MZ_ERR_ARG, "mz_select_pow_plan: null argument");
    if (!(temperature > 0.0)) return mz_internal_fail(MZ_ERR_ARG, "mz_select_pow_plan: temperature must be > 0");
    if (table && (table_len < 0 || table_len > kPowTableMax + 1))
        return mz_internal_fail(MZ_ERR_ARG, "mz_select_pow_plan: table_len outside 0..MZ_SELECT_POW_TABLE_MAX + 1");
    const HostPowPlan hp = host_pow_plan(temperature);
    *ipow = hp.ipow;
    *exact_max = hp.exact_max;
    *uses_table = hp.needs_table ? 1 : 0;
    if (table) fill_pow_table(hp.e, table, table_len);
    return MZ_OK;
}

int mz_eps_greedy(mz_batch *b, const int32_t *legal, int64_t legal_stride, float eps, const float *u_eps,
                  const double *u_cat, int32_t *action_io) {
    int B = 0, A = 0;
    hipStream_t stream = nullptr;
    int rc = consumer_info(b, &B, &A, &stream);
    if (rc) return rc;
    if (!legal || !u_eps || !u_cat || !action_io) return mz_internal_fail(MZ_ERR_ARG, "mz_eps_greedy: null buffer");
    if (legal_stride < A) return mz_internal_fail(MZ_ERR_ARG, "mz_eps_greedy: legal rows hold fewer than A entries");
    hipLaunchKernelGGL(k_eps_greedy, dim3((B + kLanes - 1) / kLanes), dim3(kLanes), 0, stream, B, A,
                       (const int *)legal, (long long)legal_stride, eps, u_eps, u_cat, (int *)action_io);
    mz_internal_enqueued(b);
    return launch_status();
}

int mz_marginal_policy(mz_batch *b, const int32_t *marginal, int64_t marginal_stride, const int32_t *legal,
                       int64_t legal_stride, int mode, int32_t *action_io, double *prob_io, double *entropy_out) {
    int B = 0, A = 0;
    hipStream_t stream = nullptr;
    int rc = consumer_info(b, &B, &A, &stream);
    if (rc) return rc;
    if (mode == MZ_MARGINAL_ARGMAX_LEGAL) {  // action_io only: prob_io and entropy_out may be NULL
        if (!marginal || !legal || !action_io) return mz_internal_fail(MZ_ERR_ARG, "mz_marginal_policy: null buffer");
        if (marginal_stride < A || legal_stride < A)
            return mz_internal_fail(MZ_ERR_ARG, "mz_marginal_policy: rows hold fewer than A entries");
        hipLaunchKernelGGL(k_marginal_argmax_legal, dim3((B + kLanes - 1) / kLanes), dim3(kLanes), 0, stream, B, A,
                           (const int *)marginal, (long long)marginal_stride, (const int *)legal,
                           (long long)legal_stride, (int *)action_io);
        mz_internal_enqueued(b);
        return launch_status();
    }
    if (mode != MZ_MARGINAL_GIVEN && mode != MZ_MARGINAL_ARGMAX)
        return mz_internal_fail(MZ_ERR_ARG, "mz_marginal_policy: bad mode");
    if (!marginal || !action_io || !prob_io || (mode == MZ_MARGINAL_ARGMAX && !legal))
        return mz_internal_fail(MZ_ERR_ARG, "mz_marginal_policy: null buffer");
    if (marginal_stride < A || (mode == MZ_MARGINAL_ARGMAX && legal_stride < A))
        return mz_internal_fail(MZ_ERR_ARG, "mz_marginal_policy: rows hold fewer than A entries");
    hipLaunchKernelGGL(k_marginal_policy, dim3((B + kLanes - 1) / kLanes), dim3(kLanes), 0, stream, B, A,
                       (const int *)marginal, (long long)marginal_stride, (const int *)legal, (long long)legal_stride,
                       mode, (int *)action_io, prob_io, entropy_out);
    mz_internal_enqueued(b);
    return launch_status();
}

int mz_value_targets(mz_batch *b, void *stream, int mode, int64_t row0, int n, int G, int U, const float *value,
                     const double *td_pow, const int32_t *td, const int32_t *pos, const int32_t *traj_len,
                     const int32_t *reward_len, const void *rewards, int rewards_f32, const void *stored,
                     int stored_f32, int64_t L, const double *dpow, const float *dpow32, int td_max,
                     double *out_value, double *out_reward) {
    hipStream_t s = nullptr;
    int rc = target_stream(b, stream, &s);
    if (rc) return rc;
    if (mode != MZ_VALUE_RE && mode != MZ_VALUE_NON_RE) return mz_internal_fail(MZ_ERR_ARG, "mz_value_targets: bad mode");
    if (!td || !pos || !traj_len || !reward_len || !rewards || !dpow || !dpow32 || !out_value || !out_reward ||
        (mode == MZ_VALUE_RE && (!value || !td_pow)) || (mode == MZ_VALUE_NON_RE && !stored))
        return mz_internal_fail(MZ_ERR_ARG, "mz_value_targets: null buffer");
    if (G < 1 || U < 0 || L < 1 || td_max < 1)
        return mz_internal_fail(MZ_ERR_ARG, "mz_value_targets: G, L, td_max must be >= 1 and U >= 0");
    if (n < 1 || row0 < 0 || row0 + n > (int64_t)G * (U + 1))
        return mz_internal_fail(MZ_ERR_ARG, "mz_value_targets: rows [row0, row0 + n) outside the G * (U + 1) rows");
    const dim3 grid((n + kLanes - 1) / kLanes), block(kLanes);
#define MZ_VT_LAUNCH(R, S)                                                                                        \
    hipLaunchKernelGGL((k_value_targets<R, S>), grid, block, 0, s, mode, (long long)row0, n, G, U + 1, value,     \
                       td_pow, (const int *)td, (const int *)pos, (const int *)traj_len, (const int *)reward_len, \
                       (const R *)rewards, (const S *)stored, (long long)L, dpow, dpow32, td_max, out_value,      \
                       out_reward)
    if (rewards_f32 && stored_f32) MZ_VT_LAUNCH(float, float);
    else if (rewards_f32) MZ_VT_LAUNCH(float, double);
    else if (stored_f32) MZ_VT_LAUNCH(double, float);
    else MZ_VT_LAUNCH(double, double);
#undef MZ_VT_LAUNCH
    if (b) mz_internal_enqueued(b);
    return launch_status();
}

int mz_pairwise_plan(int n, int32_t *starts, int32_t *ops, int cap, int32_t *num_leaves, int32_t *num_ops) {
    if (!starts || !ops || !num_leaves || !num_ops) return mz_internal_fail(MZ_ERR_ARG, "mz_pairwise_plan: null argument");
    PairwisePlan plan;
    if (!pairwise_plan(n, plan)) return mz_internal_fail(MZ_ERR_UNSUPPORTED, "mz_pairwise_plan: n outside 1..65536");
    const int nl = (int)plan.starts.size() - 1;
    if (cap < nl) return mz_internal_fail(MZ_ERR_ARG, "mz_pairwise_plan: cap below the number of leaves");
    std::copy(plan.starts.begin(), plan.starts.end(), starts);
    std::copy(plan.ops.begin(), plan.ops.end(), ops);
    *num_leaves = nl;
    *num_ops = (int)plan.ops.size();
    return MZ_OK;
}

int mz_normalize_advantage(mz_batch *b, void *stream, const float *q, const float *pred, const uint8_t *mask, int n,
                           double *adv_out, double *stats_out) {
    hipStream_t s = nullptr;
    int rc = target_stream(b, stream, &s);
    if (rc) return rc;
    if (!q || !pred || !mask || !adv_out || !stats_out)
        return mz_internal_fail(MZ_ERR_ARG, "mz_normalize_advantage: null buffer");
    if (n < 1) return mz_internal_fail(MZ_ERR_ARG, "mz_normalize_advantage: n must be >= 1");
    if (n > kAdvMaxN) return mz_internal_fail(MZ_ERR_UNSUPPORTED, "mz_normalize_advantage: n > 65536");
    DevicePlan plan;
    rc = device_plan(n, s, &plan);
    if (rc) return rc;
    hipLaunchKernelGGL(k_normalize_advantage, dim3(1), dim3(kAdvThreads), 0, s, n, q, pred, mask,
                       (const int *)plan.buf, (const int *)plan.buf + plan.nl + 1, plan.nl, plan.nops, adv_out,
                       stats_out);
    if (b) mz_internal_enqueued(b);
    return launch_status();
}

}  // extern "C"
