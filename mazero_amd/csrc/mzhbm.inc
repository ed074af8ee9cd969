// mzhbm.inc — the HBM-resident simulation step (included by mzmcts.hip inside its anonymous
// namespace; it uses that file's device helpers).
//
// Every other step kernel stages a tree's node records into LDS, so its pool must fit one CU's
// 160 KB.  The reference has no such bound: CTree_batch allocates K * (S + 2) nodes for any K and S
// (cnode.cpp:553-577, :562), e.g. A = 64, K = 70, S = 60 (3,905 reachable nodes) or 27m at K = 16,
// S = 200 (3,217).  k_hbm takes those pools: node records, value entries and the path stay in the
// arena and are read where they lie, one workgroup per tree, eight waves:
//   phase A   wave 0 expands the leaf (CTree::expand, cnode.cpp:224-295) while wave 1
//             back-propagate the path (cnode.cpp:415-450, SubTreeValueSet::update utils.cpp:20-71)
//             in chunks of 64 levels, one lane per path node: the order statistics of the node's
//             sorted (depth, value) entries by three interleaved binary searches, the node's scalars,
//             the sorted insert (the tail moved up by one, eight entries per round trip);
//   barrier   (workgroup release / acquire: the waves share the CU's L1, so the plain stores of
//             phase A are what phase B reads)
//   phase B   all eight waves recompute the min/max normaliser (CMinMaxStats, utils.cpp:79-103) over
//             the q of every visited non-root node, four 64-node blocks in flight per wave;
//   phase C   wave 0 selects (select_path / select_child / ucb_score, cnode.cpp:297-413) level by
//             level, lane j scoring child j from the records in HBM, and gathers the leaf's row.
// The arithmetic is k_step's, operation for operation (the pUCT coefficient from the pb / sq tables
// in double, the sequential arg-max with epsilon ties in closed form), so results are bit-identical
// to the LDS kernels and to the reference.
// ------------------------------------------------------------------------------------------------

// eight waves: the expansion on wave 0, the path's nodes dealt over the other seven (one node each
// up to seven levels), the min/max pass over all eight
constexpr int kHbmWaves = 8;

// The bootstrap values of path levels [lo, hi] (chunk of <= 64 levels topped by `carry` at level hi)
// and, per lane, the path node of level lev = hi - 63 + l: its record and the (already updated)
// reward of the level above (boot_dpp's layout: lane 63 holds level hi).
__device__ __forceinline__ void hbm_backup_node(const Geo &g, const Dev &d, int t, int D, int lev, int n, int nv,
                                                int4 a4, int4 b4, float4 c4, float pp, float key, float reward,
                                                float disc, int &err, long long &ent_r, long long &ent_w) {
    const size_t nb = (size_t)t * g.P;
    const int dep = D - lev;
    const float lp = d.lp()[dep];
    int2 *G = d.V() + (nb + (size_t)n) * g.E;
    // entries of a smaller depth (lo), of the same depth (c), of the same depth and a smaller value
    // (pv): nodes whose deepest entry lies above this depth append (lo = nv, c = pv = 0) without
    // reading any (utils.cpp:22-27: a new depth class)
    int lo = nv, c = 0, pv = 0;
    if (nv > 0 && md_of(b4.y) >= dep) {
        // three lower bounds over G[0, nv), sorted by (depth, value): first depth >= dep, first
        // depth > dep, first (depth, value) >= (dep, key)
        int a0 = 0, a1 = nv, b0 = 0, b1 = nv, c0 = 0, c1 = nv;
        while (a0 < a1 || b0 < b1 || c0 < c1) {
            const int ma = (a0 + a1) >> 1, mb = (b0 + b1) >> 1, mc = (c0 + c1) >> 1;
            const int2 ea = (a0 < a1) ? G[ma] : make_int2(0, 0);
            const int2 eb = (b0 < b1) ? G[mb] : make_int2(0, 0);
            const int2 ec = (c0 < c1) ? G[mc] : make_int2(0, 0);
            if (a0 < a1) {
                if (ea.x < dep) a0 = ma + 1;
                else a1 = ma;
            }
            if (b0 < b1) {
                if (eb.x <= dep) b0 = mb + 1;
                else b1 = mb;
            }
            if (c0 < c1) {
                if (ec.x < dep || (ec.x == dep && i2f(ec.y) < key)) c0 = mc + 1;
                else c1 = mc;
            }
        }
        lo = a0;
        c = b0 - a0;
        pv = c0 - a0;
        ent_r += nv;
    }
    float ws = c4.x, tw = c4.y;
    const int cur = (c == 0) ? 0 : value_lim(c, g.one_minus_rho);
    const int nl = value_lim(c + 1, g.one_minus_rho);
    if (cur == nl) {
        const float mb = i2f(G[lo + c - cur].y);  // *big.begin()
        if (!(key < mb)) {
            ws -= lp * mb;
            tw -= lp;
            tw += lp;
            ws += lp * key;
        }
    } else {
        if (cur + 1 != nl) err |= kErrValueSet;
        if (c - cur == 0) {
            tw += lp;
            ws += lp * key;
        } else {
            const float ms = i2f(G[lo + c - cur - 1].y);  // *(--small.end())
            if (key > ms) {
                tw += lp;
                ws += lp * key;
            } else {
                tw += lp;
                ws += lp * ms;
            }
        }
    }
    // insert (dep, key) at its sorted place: the tail [pos, nv) moves up by one, from the top
    const int pos = lo + pv;
    if (nv + 1 > g.E) {
        err |= kErrPath;
    } else {
        int k = nv;
        while (k > pos) {
            const int m = (k - pos) < 8 ? (k - pos) : 8;
            int2 r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < m) r[u] = G[k - 1 - u];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < m) G[k - u] = r[u];
            k -= m;
        }
        G[pos] = make_int2(dep, f2i(key));
        ent_w += nv - pos + 1;
    }
    // the node's scalars (the leaf's reward is this simulation's input; its structure record belongs
    // to the expanding wave)
    const bool is_leaf = (lev == D);
    if (is_leaf) a4.w = f2i(reward);
    const int ncn = is_leaf ? 1 : nc_of(b4.y);
    const float val = (ncn > 0) ? ws / tw : 0.f;  // CNode::value (cnode.cpp:42-56)
    const size_t gi = nb + (size_t)n;
    d.A()[gi] = make_int4(a4.x + 1, a4.y, f2i(val), a4.w);
    d.C()[gi] = make_float4(ws, tw, 0.f, 0.f);
    if (dep > md_of(b4.y) && !is_leaf) d.Bn()[gi] = make_int4(b4.x, pack_y(ncn, act_of(b4.y), dep), b4.z, b4.w);
    if (lev >= 1) d.Q()[gi] = (i2f(a4.w) + disc * val) - pp;  // get_qsa - father->pred_value
}

// One path node's update by a whole wave (all arguments wave-uniform): its sorted (depth, value)
// entries read lane-parallel -- up to kHbmRegE in registers, one round trip -- the order statistics
// counted by ballots (as bk_levels: on entries sorted by (depth, value) the counts are the three
// lower bounds of hbm_backup_node), the node's scalars, and the entries past the insertion point
// stored one place up from the registers.  Nodes with more entries take two batched passes.
constexpr int kHbmRegE = 8 * kWave;
__device__ __forceinline__ void hbm_node_wave(const Geo &g, const Dev &d, int t, int D, int lev, int n, int nv,
                                              int4 a4, int4 b4, float2 cw, float pp, float key, float reward,
                                              float disc, int &err, long long &ent_r, long long &ent_w) {
    const int l = lane_id();
    const size_t nb = (size_t)t * g.P;
    const int dep = D - lev;
    const float lp = ldsc(d.lp() + dep);
    int2 *G = d.V() + (nb + (size_t)n) * g.E;
    const bool inreg = nv <= kHbmRegE;
    int2 e[8];
    if (inreg) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = kWave * u + l;
            e[u] = (i < nv) ? G[i] : make_int2(0x7fffffff, 0);
        }
    }
    int lo = nv, c = 0, pv = 0;
    if (nv > 0 && md_of(b4.y) >= dep) {
        lo = 0;
        if (inreg) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool on = kWave * u + l < nv;
                lo += __popcll(ballot(on && e[u].x < dep));
                c += __popcll(ballot(on && e[u].x == dep));
                pv += __popcll(ballot(on && e[u].x == dep && i2f(e[u].y) < key));
            }
        } else {
            for (int e0 = 0; e0 < nv; e0 += kHbmRegE) {
                int2 f[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = e0 + kWave * u + l;
                    f[u] = (i < nv) ? G[i] : make_int2(0x7fffffff, 0);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const bool on = e0 + kWave * u + l < nv;
                    lo += __popcll(ballot(on && f[u].x < dep));
                    c += __popcll(ballot(on && f[u].x == dep));
                    pv += __popcll(ballot(on && f[u].x == dep && i2f(f[u].y) < key));
                }
            }
        }
        lo = uni(lo);
        c = uni(c);
        pv = uni(pv);
        if (l == 0) ent_r += nv;  // (the caller sums its lanes)
    }
    // entry idx's value (wave-uniform index): from the registers, else one load
    auto value_at = [&](int idx) -> float {
        if (inreg) {
            int v = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u == (idx >> 6)) v = rl(e[u].y, idx & (kWave - 1));
            return i2f(uni(v));
        }
        return i2f(uni(G[idx].y));
    };
    float ws = cw.x, tw = cw.y;
    const int cur = (c == 0) ? 0 : value_lim(c, g.one_minus_rho);
    const int nl = value_lim(c + 1, g.one_minus_rho);
    if (cur == nl) {  // SubTreeValueSet::update (utils.cpp:20-71)
        const float mb = value_at(lo + c - cur);  // *big.begin()
        if (!(key < mb)) {
            ws -= lp * mb;
            tw -= lp;
            tw += lp;
            ws += lp * key;
        }
    } else {
        if (cur + 1 != nl) err |= kErrValueSet;
        if (c - cur == 0) {
            tw += lp;
            ws += lp * key;
        } else {
            const float ms = value_at(lo + c - cur - 1);  // *(--small.end())
            if (key > ms) {
                tw += lp;
                ws += lp * key;
            } else {
                tw += lp;
                ws += lp * ms;
            }
        }
    }
    // insert (dep, key) at its sorted place: the entries [pos, nv) one place up
    const int pos = lo + pv;
    if (nv + 1 > g.E) {
        err |= kErrPath;
    } else {
        if (inreg) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = kWave * u + l;
                if (i >= pos && i < nv) G[i + 1] = e[u];
            }
        } else {  // from the top down, one batch's loads landed before its stores
            for (int top = nv; top > pos; top -= kHbmRegE) {
                const int bot = (top - kHbmRegE > pos) ? top - kHbmRegE : pos;
                int2 f[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = bot + kWave * u + l;
                    if (i < top) f[u] = G[i];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int i = bot + kWave * u + l;
                    if (i < top) G[i + 1] = f[u];
                }
            }
        }
        if (l == 0) {
            G[pos] = make_int2(dep, f2i(key));
            ent_w += nv - pos + 1;
        }
    }
    // the node's scalars (the leaf's reward is this simulation's input; its structure record belongs
    // to the expanding wave)
    const bool is_leaf = (lev == D);
    if (is_leaf) a4.w = f2i(reward);
    const int ncn = is_leaf ? 1 : nc_of(b4.y);
    const float val = (ncn > 0) ? ws / tw : 0.f;  // CNode::value (cnode.cpp:42-56)
    if (l == 0) {
        const size_t gi = nb + (size_t)n;
        d.A()[gi] = make_int4(a4.x + 1, a4.y, f2i(val), a4.w);
        d.C()[gi] = make_float4(ws, tw, 0.f, 0.f);
        if (dep > md_of(b4.y) && !is_leaf) d.Bn()[gi] = make_int4(b4.x, pack_y(ncn, act_of(b4.y), dep), b4.z, b4.w);
        if (lev >= 1) d.Q()[gi] = (i2f(a4.w) + disc * val) - pp;  // get_qsa - father->pred_value
    }
}

// CTree::back_propagate (cnode.cpp:415-450) over the path record d.path()[t], by back-propagation
// wave k of nw: chunks of 64 levels from the leaf up; in each, the bootstrap recurrence
// b_{i-1} = r_i + discount * b_i by boot_dpp (every wave computes it).  A chunk of at most
// kHbmWaveLevels levels is updated node by node, each node by a whole wave (hbm_node_wave), its levels
// dealt round-robin to the nw waves; a longer chunk (deep chains) one lane per level, by wave 0 of
// the nw (hbm_backup_node: binary searches and a serial tail move per lane, 64 nodes at once).
constexpr int kHbmWaveLevels = 16;
__device__ void hbm_backup(const Geo &g, const Dev &d, int t, int D, float value, float reward, float disc, int k,
                           int nw, int &err, long long &ent_r, long long &ent_w) {
    const int l = lane_id();
    const size_t nb = (size_t)t * g.P;
    const int2 *gp = d.path() + (size_t)t * g.PS;
    float carry = value;
    int hi = D;
    while (true) {
        const int lo = hi > 63 ? hi - 63 : 0;
        const int nl = hi - lo;
        const int lev = hi - 63 + l;
        const bool in = lev >= lo && lev <= hi;
        int n = 0, nv = 0;
        int4 a4 = make_int4(0, 0, 0, 0), b4 = a4;
        float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float pp = 0.f;
        bool ok = true;
        if (in) {
            const int2 pe = gp[lev];
            n = pe.x;
            nv = pe.y;
            ok = n >= 0 && n < g.P && nv >= 0 && nv <= g.E;  // (a path record from another search: refuse)
            if (ok) {
                a4 = d.A()[nb + n];
                b4 = d.Bn()[nb + n];
                c4 = d.C()[nb + n];
                pp = d.PP()[nb + n];
            } else {
                err |= kErrPath;
            }
        }
        if (ballot(!ok)) {  // (every wave sees the same records: none updates anything)
            err |= kErrPath;
            break;
        }
        // reward of the level above this lane's: lane l + 1's node (rewards are fixed once a node
        // is expanded; the leaf's is this simulation's input)
        const int wup = __shfl_down(a4.w, 1, kWave);
        float rn = 0.f;
        if (lev >= lo && lev < hi) rn = (lev + 1 == D) ? reward : i2f(wup);
        float b = (l == 63) ? carry : 0.f;
        float tmp = (l == 62) ? disc * carry : 0.f;
        boot_dpp(b, tmp, disc, rn, nl);
        // level lo is the next chunk's top (recomputed there as its carry): updated once, there
        const int first = (lo == 0) ? lo : lo + 1;
        if (hi - first + 1 <= kHbmWaveLevels) {
            for (int v = first + k; v <= hi; v += nw) {
                const int ln = v - hi + 63;  // its lane
                const int4 va = make_int4(rl(a4.x, ln), rl(a4.y, ln), rl(a4.z, ln), rl(a4.w, ln));
                const int4 vb = make_int4(rl(b4.x, ln), rl(b4.y, ln), rl(b4.z, ln), rl(b4.w, ln));
                hbm_node_wave(g, d, t, D, v, rl(n, ln), rl(nv, ln), va, vb, make_float2(rlf(c4.x, ln), rlf(c4.y, ln)),
                              rlf(pp, ln), rlf(b, ln), reward, disc, err, ent_r, ent_w);
            }
        } else if (k == 0 && in && (lev > lo || lo == 0)) {
            hbm_backup_node(g, d, t, D, lev, n, nv, a4, b4, c4, pp, b, reward, disc, err, ent_r, ent_w);
        }
        if (lo == 0) break;
        carry = rlf(b, 63 - nl);
        hi = lo;
    }
}

// select_path (cnode.cpp:381-413): level by level from the root, select_child (337-379) with
// ucb_score (297-335) for lane j = child j, records read from HBM; the path goes to d.path()[t].
__device__ void hbm_walk(const Geo &g, const Dev &d, int t, TreeHdr &h, float disc, int &err, int &out_idx,
                         int &out_act, long long *stl) {
    const int l = lane_id();
    const size_t nb = (size_t)t * g.P;
    const int4 *gA = d.A() + nb;
    const int4 *gB = d.Bn() + nb;
    const float *gPP = d.PP() + nb;
    const unsigned *gR = d.R() + (size_t)t * g.W;
    int2 *gp = d.path() + (size_t)t * g.PS;
    const bool mm_on = h.mm_cnt > 0;
    const float mmn = h.mm_min, mmx = h.mm_max;
    float den = 0.f;
    if (mm_on) {
        const float delta = mmx - mmn;
        den = (g.delta < delta) ? delta : g.delta;  // std::max(delta_lb, delta)
    }
    int x = 0, D = 0, cursor = h.cursor;
    int xv = uni(gA[0].x);
    int4 xb = uni4(gB[0]);
    const int root_hsx = xb.w;
    int par_hsx = root_hsx;
    // the path record {node, visits} in lane D (levels past 63 stored as they come): one store pass at
    // the end, not a store per level that the next level's loads would wait for (vmcnt counts both)
    int2 pth = make_int2(0, xv);
    long long nscored = 0;
    while (true) {
        x = uni(x);
        xv = uni(xv);
        cursor = uni(cursor);
        const int nc = uni(nc_of(xb.y));
        if (nc == 0) break;
        const int fc = uni(xb.x);
        // the children's records (lane j = child j, 64 at a time; more than 64 only with action
        // spaces past a wave, expand_wide), their structure records included: the chosen child's
        // visits and structure come from the same round trip
        const int nch = (nc + kWave - 1) / kWave;
        int4 ca[4], cb[4];
        float cpp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ca[j] = make_int4(0, 0, 0, 0);
            cb[j] = ca[j];
            cpp[j] = 0.f;
            const int i = kWave * j + l;
            if (j < nch && i < nc) {
                ca[j] = gA[fc + i];
                cb[j] = gB[fc + i];
                cpp[j] = gPP[fc + i];
            }
        }
        int ci = 0;
        if (x == 0 && xv <= nc) {
            ci = xv - 1;  // forced root round-robin (cnode.cpp:398-399)
        } else {
            const int np = xv - 1;  // total_children_visit_counts = node->visit_count - 1
            if (np < 0 || np >= g.PS) {
                err |= kErrTable;
                break;
            }
            nscored += nc;
            const float pbl = unif(d.pb()[np]);
            const double sqn = d.sq()[np];
            float sc[4];
            float M = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sc[j] = -INFINITY;
                if (j < nch) {
                    const int i = kWave * j + l;
                    if (i < nc) {
                        float vs = (ca[j].x == 0) ? 0.0f : ((i2f(ca[j].w) + disc * i2f(ca[j].z)) - cpp[j]);
                        if (mm_on) vs = (vs - mmn) / den;
                        if (vs < 0) vs = 0;
                        if (vs > 1) vs = 1;
                        const float pbc = (float)((double)pbl * (sqn / (double)(ca[j].x + 1)));  // cnode.cpp:313-314
                        sc[j] = pbc * i2f(ca[j].y) + vs;
                    }
                    M = fmaxf(M, unif(wave_max(sc[j])));
                }
            }
            // select_child's tie list (cnode.cpp:355-370) in closed form: the first maximum r and every
            // later child within epsilon of it; {s >= FLOAT_MIN} when no score beats FLOAT_MIN
            unsigned long long lst[4] = {0ull, 0ull, 0ull, 0ull};
            if (M > -1000000.0f) {  // FLOAT_MIN (utils.h:12)
                int r = -1;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nch) {
                        const unsigned long long first = ballot(kWave * j + l < nc && sc[j] == M);
                        if (r < 0 && first) r = kWave * j + (int)__builtin_ctzll(first);
                    }
                r = uni(r);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nch) {
                        unsigned long long b = ballot(kWave * j + l < nc && sc[j] >= M - 0.000001f);
                        if (kWave * (j + 1) <= r) b = 0ull;
                        else if (kWave * j < r) b &= ~0ull << (r - kWave * j);
                        lst[j] = b;
                    }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nch) lst[j] = ballot(kWave * j + l < nc && sc[j] >= -1000000.0f);
            }
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) cnt += __popcll(lst[j]);
            cnt = uni(cnt);
            if (cnt > 0) {  // one engine word (gen() % size); its value matters only for ties
                if (cursor >= g.W) {
                    err |= kErrRng;
                    break;
                }
                int k = 0;
                if (cnt > 1) {
                    const unsigned w = (unsigned)uni((int)gR[cursor]);
                    k = uni((int)(w % (unsigned)cnt));
                }
                ++cursor;
                // the k-th listed child in index order
                ci = -1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int pj = __popcll(lst[j]);
                    if (ci < 0 && k < pj) {
                        unsigned long long b = lst[j];
                        for (int q = k; q > 0; --q) b &= b - 1ull;
                        ci = kWave * j + (int)__builtin_ctzll(b);
                    } else if (ci < 0) {
                        k -= pj;
                    }
                }
                ci = uni(ci);
            }
        }
        if (D + 1 >= g.PS) {
            err |= kErrPath;
            break;
        }
        par_hsx = uni(xb.w);
        x = uni(fc + ci);
        ++D;
        // the chosen child's visits and structure record, from the registers of its lane
        int4 nb4 = make_int4(0, 0, 0, 0);
        int nvis = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j == (ci >> 6)) {
                const int cl = ci & (kWave - 1);
                nvis = rl(ca[j].x, cl);
                nb4 = make_int4(rl(cb[j].x, cl), rl(cb[j].y, cl), rl(cb[j].z, cl), rl(cb[j].w, cl));
            }
        xv = uni(nvis);
        xb = uni4(nb4);
        if (D < kWave) {
            if (l == D) pth = make_int2(x, xv);
        } else if (l == 0) {
            gp[D] = make_int2(x, xv);
        }
    }
    if (l <= D) gp[l] = pth;
    if (D == 0) err |= kErrRoot;
    h.cursor = cursor;
    h.D = D;
    h.leaf = x;
    out_idx = (D == 0) ? root_hsx : par_hsx;  // parent->hidden_state_index_x
    out_act = act_of(xb.y);                   // children_action of the last edge
    stl[MZ_S_SELECTS] += 1;
    stl[MZ_S_PATH_EDGES] += D;
    stl[MZ_S_SCORED] += nscored;
}

// min / max / count of q over the visited nodes among [1, tot), wave `wv` of kHbmWaves taking every
// kHbmWaves-th 64-node block, four blocks' loads in flight at a time (sixteen measured slower:
// 27m K = 16 phase B 3,760 -> 4,770 cycles)
__device__ __forceinline__ void hbm_minmax(const Dev &d, size_t nb, int tot, int wv, float &mn, float &mx, int &cv) {
    const int l = lane_id();
    const int *gv = (const int *)(d.A() + nb);  // {visit, ...} x 4 words per node
    const float *gQ = d.Q() + nb;
    constexpr int U = 4, stride = kWave * kHbmWaves;
    mn = INFINITY;
    mx = -INFINITY;
    cv = 0;
    for (int base = 1 + kWave * wv; base < tot; base += U * stride) {
        int v[U];
        float q[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int n = base + u * stride + l;
            v[u] = (n < tot) ? gv[4 * (size_t)n] : 0;
            q[u] = (n < tot) ? gQ[n] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool on = v[u] > 0;
            if (on) {
                mn = fminf(mn, q[u]);
                mx = fmaxf(mx, q[u]);
            }
            cv += __popcll(ballot(on));
        }
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
}

// One simulation step of one tree for pools of any size: [expand + back-propagate (sim s)] ->
// [select (sim s+1)] -> [gather], as k_step.  JOINT: agent_num > 1 (the leaf's [N][A] inputs and the
// expansion's per-agent CDFs / draws in dynamic LDS, hbm_lds_bytes).  WJ: the wide joint handles of
// mz_create_wide_joint (expand_joint_wide, its scratch in dynamic LDS, wide_joint_lds_bytes); the
// back-propagation, the normaliser and the walk are the same -- the walk scores up to 256 children in
// four chunks of 64 and takes the k-th listed child across them, and a joint selection's N actions come
// from J.  The WJ = false instantiations are the kernels they were without the parameter.
template <bool EB, bool SEL, bool JOINT, bool WJ = false>
__global__ __launch_bounds__(kHbmWaves * kWave) void k_hbm(const Params *__restrict__ prm, StepArgs a) {
    static_assert(!WJ || JOINT, "the wide joint expansion is a joint expansion");
    const Geo g = prm->g;
    const Dev d = prm->d;
    extern __shared__ __attribute__((aligned(16))) unsigned char hsm[];
    __shared__ float x_mn[kHbmWaves], x_mx[kHbmWaves];
    __shared__ int x_cv[kHbmWaves], x_err[kHbmWaves];
    __shared__ long long x_er[kHbmWaves], x_ew[kHbmWaves], x_cyc;
    // the expansion's distribution by LDS broadcasts (cdf_bcast; padded: cdf_long's last reads run
    // up to twelve entries past A)
    __shared__ __attribute__((aligned(16))) float x_cw[kWave + 16];
    __shared__ __attribute__((aligned(16))) double x_cp[kWave + 16];
    const int t = blockIdx.x;
    const int l = lane_id();
    const int wv = uni((int)(threadIdx.x >> 6));
    const size_t nb = (size_t)t * g.P;
    TreeHdr h;
    {
        const cTreeHdr *hp = (const cTreeHdr *)(d.hdr() + t);
        h.cursor = hp->cursor;
        h.tot = hp->tot;
        h.D = hp->D;
        h.err = hp->err;
        h.mm_cnt = hp->mm_cnt;
        h.tame = hp->tame;
        h.mm_min = hp->mm_min;
        h.mm_max = hp->mm_max;
        h.leaf = hp->leaf;
    }
    const int NO = JOINT ? g.N : 1;  // action words per root in the selection output
    if (h.err) {  // a dead tree stays dead and re-reports its error (see k_prepare)
        if (wv == 0) {
            if (l == 0) atomicOr(d.err(), h.err);
            if (SEL) {
                if (l == 0) {
                    a.idx_x[t] = 0;
                    a.idy[t] = t;
                }
                if (l < NO) a.act[(size_t)t * NO + l] = 0;
            }
        }
        return;
    }
    int err = 0;
    long long stl[MZ_S_COUNT];
#pragma unroll
    for (int k = 0; k < MZ_S_COUNT; ++k) stl[k] = 0;
    // (stamped builds: s_memtime at the phase ends, cycles per launch and tree into the stats slots)
    unsigned long long ts[8] = {0};
    stamp(ts, 0);
    const int tot = h.tot;
    if (EB) {
        const float r_in = a.reward[t], v_in = a.value[t];
        if (wv == 0) {
            // ---- CTree::expand (cnode.cpp:224-295) of the leaf (expand_and_backprop, :452-469) ----
            const int leaf = h.leaf;
            const int4 leaf_b = d.Bn()[nb + leaf];
            int cursor = h.cursor, ntot = tot;
            long long st_new = 0;
            int nc;
            if constexpr (WJ) {
                const size_t ib = (size_t)t * g.NA;
                nc = expand_joint_wide(g, d, t, leaf, a.policy + ib, a.beta + ib, nullptr, 0.f, a.K, v_in, cursor, ntot,
                                       hsm, err, st_new);
                h.tame = 0;
            } else if (JOINT) {
                const int NA = g.NA;
                float *jp = (float *)hsm, *jb = jp + NA;
                double *jcp = (double *)(hsm + ((8 * NA + 15) & ~15));
                int *jd = (int *)(jcp + NA);
                const size_t ib = (size_t)t * NA;
                for (int i = l; i < NA; i += kWave) {
                    jp[i] = a.policy[ib + i];
                    jb[i] = a.beta[ib + i];
                }
                wait_lds();
                nc = expand_joint(g, d, t, leaf, jp, jb, nullptr, 0.f, a.K, v_in, cursor, ntot, nullptr, 0, nullptr,
                                  nullptr, jcp, jd, err, st_new);
                h.tame = 0;
            } else if (g.A > kMaxActions) {  // more actions than lanes
                const size_t ib = (size_t)t * g.A;
                int wild = 0;
                nc = expand_wide(g, d, t, leaf, a.policy + ib, a.beta + ib, nullptr, 0.f, a.K, v_in, cursor, ntot, err,
                                 st_new, wild);
                if (wild || !tame_val(v_in) || !tame_val(r_in)) h.tame = 0;
            } else {
                const size_t ib = (size_t)t * g.A;
                // the first 64 draws' engine words, issued with the leaf's inputs: they land while the
                // distribution is built (expand_node would read them after it)
                unsigned w1r = 0u, w2r = 0u;
                if (g.A >= 2 && l < a.K) {
                    w1r = rng_word_lane(g, d, nullptr, 0, t, cursor + 2 * l, err);
                    w2r = rng_word_lane(g, d, nullptr, 0, t, cursor + 2 * l + 1, err);
                }
                const float pol = (l < g.A) ? a.policy[ib + l] : 0.f;
                const float bet = (l < g.A) ? a.beta[ib + l] : 0.f;
                int wild = 0;
                nc = expand_node(g, d, t, leaf, pol, bet, 0.f, 0.f, a.K, v_in, cursor, ntot, nullptr, 0, nullptr, err,
                                 st_new, true, w1r, w2r, MZ_STAMPS ? stl : nullptr, wild, nullptr, x_cw, x_cp);
                if (wild || !tame_val(v_in) || !tame_val(r_in)) h.tame = 0;
            }
            stl[MZ_S_EXPANDS] += 1;
            stl[MZ_S_NEW_CHILDREN] += st_new;
            // (an engine-stream overrun is flagged by the lanes that drew past it: wave-uniform from here)
            for (unsigned long long m = ballot(err != 0); m; m &= m - 1ull) err |= rl(err, __builtin_ctzll(m));
            err = uni(err);
            if (!err && l == 0) {
                // the leaf's structure: first child, children count, (maxdepth >= 0 after this
                // simulation's back-propagation), pred_value, hidden_state_index_x
                const int md = md_of(leaf_b.y) < 0 ? 0 : md_of(leaf_b.y);
                d.Bn()[nb + leaf] = make_int4(tot, pack_y(nc, act_of(leaf_b.y), md), f2i(v_in), a.hsx);
            }
            if (!err) {
                h.cursor = cursor;
                h.tot = ntot;
            }
            stamp(ts, 1);
        } else {
            // ---- CTree::back_propagate (cnode.cpp:415-450), waves 1 .. kHbmWaves - 1 ----
            long long er = 0, ew = 0;
            hbm_backup(g, d, t, h.D, v_in, r_in, a.discount, wv - 1, kHbmWaves - 1, err, er, ew);
            for (unsigned long long m = ballot(err != 0); m; m &= m - 1ull) err |= rl(err, __builtin_ctzll(m));
            stamp(ts, 1);
            if (l == 0) {
                x_err[wv] = err;
                x_er[wv] = wave_sum((int)er);
                x_ew[wv] = wave_sum((int)ew);
                if (wv == 1) x_cyc = (long long)(ts[1] - ts[0]);
            }
        }
        __syncthreads();  // (release / acquire: the back-propagation's stores are what phase B reads)
        stamp(ts, 2);
        // ---- the min/max normaliser over every visited non-root node (utils.cpp:79-103); this
        // simulation's new children are unvisited, so nodes [1, tot) ----
        float mn, mx;
        int cv;
        hbm_minmax(d, nb, tot, wv, mn, mx, cv);
        if (l == 0) {
            x_mn[wv] = mn;
            x_mx[wv] = mx;
            x_cv[wv] = cv;
        }
        lds_barrier();
        if (wv != 0) return;
        stamp(ts, 3);
#pragma unroll
        for (int w = 1; w < kHbmWaves; ++w) {
            err |= uni(x_err[w]);
            stl[MZ_S_ENTRIES_READ] += x_er[w];
            stl[MZ_S_ENTRIES_WRITTEN] += x_ew[w];
        }
        stl[MZ_S_BACKUP_NODES] += h.D + 1;
        if (MZ_STAMPS) stl[MZ_S_CYC_W1_BACKUP] += x_cyc;  // wave 1: the back-propagation
        float m0 = x_mn[0], m1 = x_mx[0];
        int c0 = x_cv[0];
#pragma unroll
        for (int w = 1; w < kHbmWaves; ++w) {
            m0 = fminf(m0, x_mn[w]);
            m1 = fmaxf(m1, x_mx[w]);
            c0 += x_cv[w];
        }
        const bool moved = c0 > 0 && (h.mm_cnt == 0 || f2i(unif(m0)) != f2i(h.mm_min) || f2i(unif(m1)) != f2i(h.mm_max));
        if (moved) stl[MZ_S_MM_MOVED] += 1;
        h.mm_min = unif(m0);
        h.mm_max = unif(m1);
        h.mm_cnt = uni(c0);
        stl[MZ_S_MINMAX_NODES] += tot - 1;
    } else if (wv != 0) {
        return;
    }
    // ---- selection (wave 0) ----
    if (!SEL) stamp(ts, 4);
    if (SEL) {
        int idx = 0, act = 0;
        if (!err) hbm_walk(g, d, t, h, a.discount, err, idx, act, stl);
        stamp(ts, 4);
        if (l == 0) {
            a.idx_x[t] = err ? 0 : idx;
            a.idy[t] = t;
        }
        if (JOINT) {
            if (l < g.N) a.act[(size_t)t * g.N + l] = err ? 0 : (int)d.J()[(size_t)t * g.JP + (size_t)h.leaf * g.N + l];
        } else if (l == 0) {
            a.act[t] = err ? 0 : act;
        }
        if (a.pool && !err) {  // mcts_sampled.py:130-134: leaf hidden state = pool[idx_x][t]
            const char *src = a.pool + (long long)idx * a.pool_stride + (long long)t * a.row_bytes;
            char *dst = a.gather_out + (long long)t * a.row_bytes;
            const long long rb = a.row_bytes;
            if (((rb | (long long)(uintptr_t)src | (long long)(uintptr_t)dst) & 15) == 0) {
                // sixteen 16-byte loads per lane in flight (16 KiB per round trip), then their stores,
                // written through (st_wt16: the rows are most of a launch's stores, see k_chain3)
                for (long long o0 = (long long)l * 16; o0 < rb; o0 += 16 * 16 * kWave) {
                    int4 v[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const long long o = o0 + (long long)u * 16 * kWave;
                        if (o < rb) v[u] = *(const int4 *)(src + o);
                    }
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const long long o = o0 + (long long)u * 16 * kWave;
                        if (o < rb) st_wt16(dst + o, v[u]);
                    }
                }
            } else {
                for (long long o = (long long)l * 4; o < rb; o += 4 * kWave) *(int *)(dst + o) = *(const int *)(src + o);
            }
        }
    }
    // header (scalars from lane 0; the engine words for the next expansion are not carried: k_hbm
    // reads them from the stream itself)
    if (l == 0) {
        TreeHdr *hp = d.hdr() + t;
        hp->cursor = h.cursor;
        hp->tot = h.tot;
        hp->D = h.D;
        hp->err = err;
        hp->mm_min = h.mm_min;
        hp->mm_max = h.mm_max;
        hp->mm_cnt = h.mm_cnt;
        hp->tame = h.tame;
        hp->leaf = h.leaf;
        hp->hot_tag = 0;  // (k_chain3's copy of A[root].x / Bn[leaf].y: not maintained here)
    }
    stamp(ts, 5);
    long long *st = d.stats() + (size_t)t * MZ_S_COUNT;
    if (MZ_STAMPS) {
        stl[MZ_S_CYC_EXPAND] += (long long)(ts[1] - ts[0]);     // wave 0: the expansion
        stl[MZ_S_CYC_BACKUP] += (long long)(ts[2] - ts[0]);     // phase A (the barrier left)
        stl[MZ_S_CYC_MINMAX] += (long long)(ts[3] - ts[2]);     // phase B
        stl[MZ_S_CYC_SELECT] += (long long)(ts[4] - ts[3]);     // the walk
        stl[MZ_S_CYC_EPILOGUE] += (long long)(ts[5] - ts[4]);   // gather, header
        stl[MZ_S_STAMPED] += 1;
    }
    if (l == 0) {
#pragma unroll
        for (int k = 0; k < (MZ_STAMPS ? MZ_S_COUNT : MZ_S_CYC_HEADER); ++k) st[k] += stl[k];
        if (err) atomicOr(d.err(), err);
    }
}

// dynamic LDS of k_hbm: the joint expansion's staged [N][A] policy and beta, per-agent CDFs and the
// draws (agent_num > 1 only)
int hbm_lds_bytes(int N, int NA) {
    if (N <= 1) return 0;
    return ((8 * NA + 15) & ~15) + 8 * NA + 4 * kWave * N;
}
