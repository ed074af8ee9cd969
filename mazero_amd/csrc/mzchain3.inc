// mzchain3.inc — K = 1 chains on three wave roles and a draw wave: ChainK / ChainIO / Chain3Args,
// the scalar-load helpers (sload*), Chain3Layout, the draw slot, draw_u and k_chain3.  Included by
// mzmcts.hip inside its anonymous namespace.
//
// Uses: of what stands above its include line, only the shared definitions at the top of
// mzmcts.hip (Dev, TreeHdr, RbDesc and readback_emit, the arena offsets, cdf_lane / cdf_short /
// cdf_bcast, the wave primitives, the spans, MZ_STAMPS) -- nothing of k_step's or k_chain's.
// Used below it: draw_u by k_prepare1; ChainK, ChainIO and k_chain3 by the host side and mz_create.
// ------------------------------------------------------------------------------------------------

// ================================================================================================
// K = 1 chains, round 3: three wave roles, the bootstrap recurrence in registers
// ================================================================================================
// The same simulation step as k_chain (expansion of the leaf, back-propagation over the chain,
// min/max normaliser, selection of the new child, leaf-row gather), re-split so that nothing but
// the expansion and the back-propagation sits on a launch's critical path:
//  - wave 0 expands the leaf (distribution, draw, the child's records), writes the selection
//    outputs and, after the one barrier, the header;
//  - wave 1 back-propagates.  Its node records arrive in registers (lane i = node i).  The
//    recurrence b_{i-1} = r_i + discount * b_i (cnode.cpp:424,448) runs in registers on every lane
//    at once (all lanes hold the same b), fed by the chain's rewards read from LDS sixteen at a
//    time: one dependent multiply + add per level instead of a DPP lane shift;
//  - wave 2 does what depends only on the header: the leaf-row gather (the next leaf's parent is
//    this launch's leaf), the next expansion's engine words when the selection is known to take
//    one word per level (every prior of the leaf's distribution tame: select_walk's fast case
//    whatever the draw), and the statistics counters.
// Every error and output is decided from the same scalar inputs as k_chain: results are bit-identical.
//
// Launch arguments.  The first 14 dwords arrive preloaded in SGPRs; they hold everything round 1
// addresses: tree t's header is a 256-byte block at a constant offset, the lambda-power table
// follows the headers (arena_lp), and the node arrays are at o_A plus constant multiples of the unit
// c (arena_nodes_at), both packed in the argument apk (arena_pack): no role computes a round-up to
// reach a record, and every record is addressed as the arena base plus a 32-bit byte offset.
// The kernel's first instructions test the wave index: each role then computes only what its first
// loads address and issues them; P, PS, the hsx range test and the rest follow behind the issue.
// The rest (ChainIO) is read through the kernel-argument pointer by the waves
// that need it, where they need it: the compiler would otherwise load every argument in the common
// prologue and wait there.  ChainIO is two 64-byte lines, one scalar load each: wave 2's (the row
// gather's arguments) and wave 0's (the output pointers), each with the handle constants that role
// would otherwise fetch from Params (ChainK, filled once at mz_create).  Wave 1 needs neither.
// Round 1's scalar loads are issued by inline assembly (sload*) and waited for with one explicit
// wait per role: the compiler would sink each load past the first branch after it.
// --------------------------------------------------------------------------------------------
struct ChainK {  // the Params fields wave 0 reads (mz_create checks them against Params)
    float one_minus_rho;
    int W;
    unsigned o_R, o_err, o_D, o_stats;
    float delta;
    unsigned o_pb, o_sq;
    float discount;  // (the launch's: waves 0 and 1 read it here, it is not among the preloaded dwords)
};
struct ChainIO {
    // wave 2's line
    const char *pool;
    long long pool_stride, row_bytes;
    char *gather_out;
    float w2_one_minus_rho;
    unsigned w2_o_stats;
    int pad_[6];
    // wave 0's line
    int *idx_x, *idy, *act;
    ChainK k;
};
struct Chain3Args {  // k_chain3's parameter list, for the kernel-argument offset of ChainIO
    char *base;
    const float *policy, *beta, *reward, *value;
    int ppk, bak, hsx, apk;
    const char *src_slot;
    ChainIO io;
};
// (the first 14 dwords, through apk, arrive preloaded in SGPRs: two of the 16 user SGPRs
// hold the kernel-argument pointer.  src_slot is not among them: wave 2 fetches it with a scalar
// load and waits for it before it issues the row's loads)
static_assert(offsetof(Chain3Args, src_slot) == 56 && offsetof(Chain3Args, io) == 64 && sizeof(ChainIO) == 128 &&
                  offsetof(ChainIO, idx_x) == 64 && sizeof(ChainK) == 40,
              "k_chain3 argument layout: one 64-byte line per role");
#ifdef __HIP_DEVICE_COMPILE__
typedef const __attribute__((address_space(4))) ChainIO cChainIO;
#else
typedef const ChainIO cChainIO;
#endif

typedef int int4v __attribute__((ext_vector_type(4)));
typedef int int8v __attribute__((ext_vector_type(8)));
typedef int int16v __attribute__((ext_vector_type(16)));
typedef float float2v __attribute__((ext_vector_type(2)));
// stores through an address a lane holds in registers (typed as global memory: global_store, not flat)
#ifdef __HIP_DEVICE_COMPILE__
typedef __attribute__((address_space(1))) int4v g_int4v;
typedef __attribute__((address_space(1))) int g_int;
typedef __attribute__((address_space(1))) float2v g_float2v;
// and through an LDS address a lane holds as a 32-bit value
typedef __attribute__((address_space(3))) int4v lds_int4v;
typedef __attribute__((address_space(3))) float2v lds_float2v;
typedef __attribute__((address_space(3))) float lds_f32;
#else
typedef int4v g_int4v;
typedef int g_int;
typedef float2v g_float2v;
typedef int4v lds_int4v;
typedef float2v lds_float2v;
typedef float lds_f32;
#endif
__device__ __forceinline__ void st_lane16(uintptr_t p, int4v v) { *(g_int4v *)p = v; }
__device__ __forceinline__ void st_lane4(uintptr_t p, int v) { *(g_int *)p = v; }
// scalar loads issued here and waited for by swait (invisible to the compiler's wait counting, which
// stays correct: its own LDS waits only ever wait longer with more loads outstanding)
template <int OFF = 0>  // (an immediate byte offset)
__device__ __forceinline__ int sload1(const void *p) {
    int v;
    asm volatile("s_load_dword %0, %1, %2" : "=s"(v) : "s"(p), "n"(OFF) : "memory");
    return v;
}
typedef int int2v __attribute__((ext_vector_type(2)));
template <int OFF = 0>  // (an immediate byte offset)
__device__ __forceinline__ int2v sload2(const void *p) {
    int2v v;
    asm volatile("s_load_dwordx2 %0, %1, %2" : "=s"(v) : "s"(p), "n"(OFF) : "memory");
    return v;
}
__device__ __forceinline__ uintptr_t u64_of(int lo, int hi) {
    return (uintptr_t)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
template <int OFF = 0>  // (an immediate byte offset)
__device__ __forceinline__ int4v sload4(const void *p) {
    int4v v;
    asm volatile("s_load_dwordx4 %0, %1, %2" : "=s"(v) : "s"(p), "n"(OFF) : "memory");
    return v;
}
template <int OFF = 0>  // (an immediate byte offset)
__device__ __forceinline__ int8v sload8(const void *p) {
    int8v v;
    asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(v) : "s"(p), "n"(OFF) : "memory");
    return v;
}
template <int OFF = 0>  // (an immediate byte offset)
__device__ __forceinline__ int16v sload16(const void *p) {
    int16v v;
    asm volatile("s_load_dwordx16 %0, %1, %2" : "=s"(v) : "s"(p), "n"(OFF) : "memory");
    return v;
}

template <int NC>
struct Chain3Layout {
    int oW, oP, oRv, oBv, oA, oPP, oX, total;
    __host__ __device__ static constexpr int r16(int x) { return (x + 15) & ~15; }
    __host__ __device__ constexpr Chain3Layout(int P)
        : oW(0),                         // float[64]  the leaf's weights (distribution broadcast)
          oP(4 * kWave),                 // double[64] its probabilities
          oRv(oP + 8 * kWave),           // float[P + 32]  rewards reversed: [j] = r_{D-j}
          oBv(oRv + r16(4 * (P + 32))),  // float[P + 32]  bootstrap values: [j] = b_{D-1-j}
          oA(oBv + r16(4 * (P + 32))),   // int4[P + 1]    node records after the back-propagation
          oPP(oA + r16(16 * (P + 1))),   // float[P + 1]   parents' pred_value
          oX(oPP + r16(4 * (P + 1))),    // min, max, wave 2's flag, v_in; stamps from 64
          total(oX + 128) {}
};
int chain3_lds_bytes(int nc) { return Chain3Layout<0>(nc).total; }

// ROW: the leaf-row gather's class -- 0 any row, 1 16-byte aligned rows of <= 4 KiB (registers), 2
// aligned rows of <= 16 KiB (LDS-DMA), 3 no gather (no pool, or no selection).  For ROW 1 and 2 the
// host passes the leaf's slot (pool + hsx * pool_stride) in the argument src_slot (the first one past
// the preloaded 14 dwords: one scalar load) and the row size in 16-byte units in the preloaded ppk's
// top bits: wave 2 issues the row's loads as soon as src_slot has landed, ahead of its scalar round.
//
// W4: a fourth wave (the draw wave) builds the expansion's distribution and draws the action from
// launch start, beside wave 0's round 1.
//
// With a selection and the role-first entry (SEL, ROW != 2: kDS in the kernel) the draw wave stores
// what it draws and the two waves never talk.  Both load the same header line, policy and beta rows,
// reward, value and arguments and evaluate one predicate (draw_pred): no error, the chain in
// sequence with a valid hot copy, and select_walk's fast case whatever the draw (every lane's prior
// tame).  When it holds, the drawn action feeds five words only -- A[child].y (the prior),
// Bn[child].y (the action), act[t], the header's leaf_y and D[child] under the root -- and the draw
// wave stores them, the two records whole; wave 0 writes everything else and ends without an action.
// When it does not hold, the draw wave returns without a store and wave 0 draws itself in registers
// (cdf_short, cdf_lane past 16 actions).  No LDS slot, no start barrier, no poll: waves 1 and 2
// never wait for another wave.  -DMZ_CHAIN3_DRAW_STORES=0 makes the predicate false everywhere (the
// tests' second build).
//
// The fused readback (SEL = false) and the 16 KiB row class (ROW = 2) keep the hand-over: there the
// draw wave needs only this launch's beta row and the header's two
// engine words, both addressed from the preloaded arguments.  It hands the action to wave 0 through
// one LDS dword (kDrawSlot of the oX region: bit 31 set, the action below it, one store).  LDS is not
// cleared between workgroups, so wave 0 clears the slot and one s_barrier, taken by all four waves
// behind their round-1 load issue and before any early return, separates the clear from the publish.
// Wave 0 polls the slot a bounded number of times (kDrawPolls); if the bound runs out it draws itself
// in registers (cdf_row, cdf_lane past 16 actions; no LDS: the draw wave may still be using sW / sP),
// bit-identical, so a launch can never hang on the hand-over.
constexpr int kDrawSlot = 4;  // dword of the oX region (0, 1: min / max; stamps from dword 16)
#ifndef MZ_CHAIN3_POLLS
#define MZ_CHAIN3_POLLS 128  // ~100 cycles each: several times the draw wave's ~2,000 cycles
#endif
constexpr int kDrawPolls = MZ_CHAIN3_POLLS;
#ifndef MZ_CHAIN3_DRAW_STORES
#define MZ_CHAIN3_DRAW_STORES 1  // 0: draw_pred false everywhere (wave 0 draws, the draw wave stores nothing)
#endif
__device__ __forceinline__ void start_barrier() { asm volatile("s_barrier" ::: "memory"); }
// the slot's accesses: volatile (every poll reads LDS again) and typed as LDS (a volatile access
// through a generic pointer is a flat one, which also waits for the wave's global stores)
#ifdef __HIP_DEVICE_COMPILE__
typedef volatile __attribute__((address_space(3))) int lds_vint;
#else
typedef volatile int lds_vint;
#endif
__device__ __forceinline__ void draw_slot_set(int *sxi, int v) { *(lds_vint *)(lds_void *)&sxi[kDrawSlot] = v; }
__device__ __forceinline__ int draw_slot_get(int *sxi) { return *(lds_vint *)(lds_void *)&sxi[kDrawSlot]; }
// the draw's u from two engine words (generate_canonical<double, 53>, libstdc++ random.tcc:3348-3378)
__device__ __forceinline__ double draw_u(unsigned n0, unsigned n1) {
    const double w1 = (double)n0, w2 = (double)n1;
    double u = (w1 + w2 * 4294967296.0) / 18446744073709551616.0;
    if (u >= 1.0) u = 0x1.fffffffffffffp-1;  // nextafter(1, 0)
    return u;
}
template <int NC, bool SEL, int ROW, bool W4>
__global__ __launch_bounds__(W4 ? 256 : 192) void k_chain3(char *base, const float *policy, const float *beta, const float *reward,
                                                const float *value, int ppk, int bak, int hsx, int apk,
                                                const char *src_slot, ChainIO io) {
    static_assert(NC >= kWave && NC % kWave == 0 && NC < 1024, "k_chain3 node classes are whole waves, < 1024");
    (void)io;  // (read through the kernel-argument pointer, see above)
    constexpr int NCH = NC / kWave;  // node chunks of one wave
    constexpr Chain3Layout<NC> L(NC);
    // The 16 KiB row class (ROW 2) keeps the entry this kernel had before the role-first one, line for
    // line: the role tests in the order 3, 1, 2, the node arrays' offsets by arena_nodes while the
    // header load is in flight, masked record loads through 64-bit addresses, and the discount in the
    // 14th preloaded dword -- in these instantiations apk carries the discount's bits
    // (launch_chain3_row).  There wave 2 issues sixteen LDS-DMA loads ahead of the start barrier, and
    // with the role-first entry 27m K = 1 measured 3.2 % slower whatever the order of the role tests
    // (profiles/chain3_entry).
    constexpr bool kEntry = ROW != 2;
    // the draw wave stores what it draws (above); the other four-wave instantiations hand over
    constexpr bool kDS = W4 && SEL && kEntry, kHand = W4 && !kDS;
    // (stamped builds: every role's phases count from its wave's first instruction)
    unsigned long long ts[8] = {0};
    stamp(ts, 0);
    const unsigned long long rt0 = span_open();
    // The role first: the wave index is tested in the kernel's first instructions, each role's body
    // lies out of line behind one taken branch (wave 0 falls through), and what follows here is
    // computed by the role that uses it, behind its first loads' issue -- nothing but the role test
    // is common to the four waves.
    const int wv = uni((int)(threadIdx.x >> 6));
    // (one compare and one branch per role: the empty asm keeps the compiler from folding the tests
    // into a search over the wave index with flag registers)
    auto role = [&](int r) {
        int w = wv;
        asm volatile("" : "+s"(w));
        return w == r;
    };
    const int t = blockIdx.x;
    const int l = threadIdx.x & (kWave - 1);
    Dev d;
    d.base = (gchar *)base;
    d.o_hdr = kArenaHdr;
    // (!kEntry) the node arrays' offsets, computed by each role after it has issued its header load
    // (the empty asm orders the arithmetic behind the loads' asm statements)
    auto arena = [&]() {
        int bk = bak, pk = ppk;
        asm volatile("" : "+s"(bk), "+s"(pk));
        arena_nodes(d, (unsigned)bk & 0xffffffu, (unsigned)pk & 0x3ffu, ((unsigned)pk >> 10) & 0x3ffu);
    };
    cChainIO *iop = (cChainIO *)((const char *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(Chain3Args, io));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *sX = (float *)(smem + L.oX);
    int *sXi = (int *)(smem + L.oX);
    long long *sXl = (long long *)(smem + L.oX + 64);
    int4 *sA = (int4 *)(smem + L.oA);
    float *sPP = (float *)(smem + L.oPP);
    float *sRv = (float *)(smem + L.oRv);
    float *sBv = (float *)(smem + L.oBv);
    // tree t's header block: 32-bit arithmetic (t < B < o_A < 65536, arena_packs) and, in the scalar
    // loads, the headers' offset as the instruction's immediate
    constexpr int kHdr8 = (int)kArenaHdr * 256;
    auto hb_of = [&]() { return (const gchar *)d.base + ((unsigned)t << 8); };
    auto hdr_of = [&](const gchar *hb) { return (TreeHdr *)(gchar *)(hb + kHdr8); };
    // (likewise the launch's inputs: t * A * 4 < 2^25)
    auto in_t = [&](const float *p) { return (const void *)((const gchar *)p + ((unsigned)t << 2)); };
    auto in_row = [&](const float *p, int A) {
        return *(const float *)((const gchar *)p + (((unsigned)t * (unsigned)A + (unsigned)(l < A ? l : 0)) << 2));
    };
    const void *ka = (const void *)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int kIo = (int)offsetof(Chain3Args, io);
    // the node arrays as 32-bit byte offsets off the arena base, from the packed argument (arena_pack:
    // the arrays end below 4 GiB)
    auto oA8_of = [&]() { return ((unsigned)apk & 0xffffu) << 8; };
    auto c8_of = [&]() { return ((unsigned)apk >> 16) << 8; };
    auto P_of = [&]() { return ppk & 0x3ff; };
    auto PS_of = [&]() { return (ppk >> 10) & 0x3ff; };
    auto A_of = [&]() { return (bak >> 24) & 0x7f; };
    // the chain's leaf, if the header agrees
    auto Dp_of = [&](int P) { return (hsx >= 0 && hsx + 1 <= P) ? hsx : 0; };
    // "not a chain", the one predicate of waves 0, 1 and 2 (all three read the same header).  A depth
    // below 0 counts as out of range: wave 1's record loads clamp their lane to D as unsigned.
    auto no_chain = [&](int D, int P, int toth, int leafh) {
        return (kEntry ? (unsigned)D >= (unsigned)P : D + 1 > P) || toth != D + 1 || leafh != D;
    };
    // (kDS) "the launch is fast whatever the draw", the one predicate of wave 0 and the draw wave:
    // both evaluate it from the same loaded words (hv: the header line; wild: the lane's prior is
    // not tame).  It implies err == 0, tame == 1 and select_walk's fast case for every action.
    auto draw_pred = [&](const int16v &hv, int omri, int disc_i, int r_i, int v_i, bool wild) {
        if (!MZ_CHAIN3_DRAW_STORES) return false;
        // Branch-free, a few dozen scalar instructions on both waves' critical paths: every equality
        // is one xor into `ne`, every bound one difference whose sign bit goes into `neg` (32-bit
        // wrap-around only ever fails a bound that held, and then wave 0 draws: the predicate is
        // sufficient, not necessary).  Floats by their bits: |x| <= c is (bits & 0x7fffffff) <=
        // bits(c), false for NaN; value_lim(1, omr) == 1 when omr's bits are at most 1.0f's (or omr
        // is at most -1.0: the wrapped difference).
        const unsigned P = (unsigned)P_of(), PS = (unsigned)PS_of(), toth = (unsigned)hv[1], D = (unsigned)hv[2];
        const unsigned kAbs = 0x7fffffffu, kTame = 0x7149f2cau /* 1e30f */, kOne = 0x3f800000u /* 1.0f */;
        // no error, the chain in sequence (D == hsx, tot, leaf), the hot copy (root_vis, leaf_y) valid
        const unsigned ne = (unsigned)hv[3] | (D ^ (unsigned)hsx) | (toth ^ (D + 1u)) | ((unsigned)hv[7] ^ D) |
                            ((unsigned)hv[11] ^ toth);
        const unsigned va = (unsigned)v_i & kAbs, ra = (unsigned)r_i & kAbs;
        unsigned neg = D | (P - 2u - D) | (PS - 2u - D);           // 0 <= D, no err1 (pool) / errp (path)
        neg |= PS - 1u - (unsigned)hv[9];                          // no table error (root_vis < PS)
        neg |= kOne - (unsigned)omri;                              // no err1 (value set)
        neg |= ~(unsigned)bak | ((unsigned)hv[8] - 1u);            // fast_ok, h.tame (0 or 1)
        neg |= kTame - (va > ra ? va : ra);                        // v_in, r_in tame
        neg |= kOne - ((unsigned)disc_i & kAbs);                   // |discount| <= 1
        return (ne | (neg >> 31)) == 0 && ballot(wild) == 0;
    };

    auto wave3 = [&]() {
        if constexpr (kDS) {
            // ======== wave 3: the expansion's distribution and draw (cnode.cpp:224-295), and the
            // stores of the words the draw feeds ========
            // Round 1 as wave 0's: the header line, this launch's rows and scalars, and of wave 0's
            // argument line what the predicate and the stores need.  When the predicate fails wave 0
            // draws and stores; this wave returns.
            if (!MZ_CHAIN3_DRAW_STORES) return;
            const int A = A_of(), P = P_of();
            constexpr int kK = kIo + (int)offsetof(ChainIO, k);
            const gchar *hb = hb_of();
            int16v hv = sload16<kHdr8>(hb);
            int2v actp = sload2<kIo + (int)offsetof(ChainIO, act)>(ka);
            int omri = sload1<kK + (int)offsetof(ChainK, one_minus_rho)>(ka);
            int oDi = sload1<kK + (int)offsetof(ChainK, o_D)>(ka);
            int g_i = sload1<kK + (int)offsetof(ChainK, discount)>(ka);
            int r_i = sload1(in_t(reward)), v_i = sload1(in_t(value));
            const float pol = in_row(policy, A), bet = in_row(beta, A);
            // lane 2 the child's A, lane 3 the child's Bn (whole records, as wave 0's lanes store them
            // when it draws); the child of an in-sequence launch is hsx + 1 (clamped here: the
            // predicate fails when hsx is out of range)
            const unsigned nd1 = (unsigned)t * (unsigned)P + (unsigned)Dp_of(P) + 1;
            const uintptr_t abase = (uintptr_t)d.base;
            uintptr_t p16 = abase + (oA8_of() + (l == 2 ? 0u : kNodeSpanBn) * c8_of() + nd1 * 16);
            asm volatile("" : "+v"(p16));
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+s"(hv), "+s"(actp), "+s"(omri), "+s"(oDi), "+s"(g_i), "+s"(r_i), "+s"(v_i)
                         :
                         : "memory");
            const float prior_l = pol * 1.0f / bet;  // (betahat_prob = 1, as wave 0's priors())
            if (!draw_pred(hv, omri, g_i, r_i, v_i, !tame_prior(prior_l))) return;
            int a = 0;
            if (A >= 2) {
                const double cp = (A <= 16) ? cdf_short(A, (l < A) ? bet : 0.f)
                                            : cdf_bcast(bet, A, (float *)(smem + L.oW), (double *)(smem + L.oP));
                const double u = draw_u((unsigned)hv[12], (unsigned)hv[13]);
                a = __popcll(ballot(l < A && cp < u));  // lower_bound
            }
            a = uni(a);
            const int by = pack_y(0, a, -1);
            const float prior = rlf(prior_l, a);
            const int4v d16 = {0, l == 2 ? f2i(prior) : by, 0, l == 3 ? -1 : 0};
            if (l == 2 || l == 3) st_lane16(p16, d16);
            if (l == 3) st_lane4((uintptr_t)u64_of(actp[0], actp[1]) + ((unsigned)t << 2), a);
            if (hv[2] == 0) {  // (readbacks: root children)
                const float pol_a = rlf(pol, a), bet_a = rlf(bet, a);
                d.o_D = (unsigned)oDi;
                if (l == 0) d.D()[(size_t)nd1] = make_float4(pol_a, bet_a, 1.0f, 0.f);
            }
            if (l == 0) {
                hdr_of(hb)->leaf_y = by;
                if (MZ_STAMPS) sXl[3] = (long long)(__builtin_amdgcn_s_memtime() - ts[0]);  // this wave's end
            }
            wait_lds();
        } else if constexpr (W4) {
            const int A = A_of();
            // ======== wave 3 (the hand-over): the expansion's distribution and draw (cnode.cpp:224-295) ========
            // Straight-line code: this launch's beta row and the header's two engine words, the
            // start barrier while they are in flight, the distribution, one LDS store.  No header
            // check (on a dead or out-of-chain tree wave 0 returns before it reads the slot; the
            // loads are in bounds for every t), no global store.
            float bet;
            int2v nx;
            if constexpr (kEntry) {
                bet = in_row(beta, A);
                nx = sload2<kHdr8 + (int)offsetof(TreeHdr, nxt)>(hb_of());
            } else {
                bet = beta[(size_t)t * A + (l < A ? l : 0)];
                nx = sload2(&(d.hdr() + t)->nxt[0]);
            }
            start_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(nx) : : "memory");
            int a = 0;
            if (A >= 2) {
                // (up to 16 actions in registers, cdf_row: this wave has nothing to hide behind LDS waits)
                const double cp = (A <= 16) ? cdf_short(A, (l < A) ? bet : 0.f)
                                            : cdf_bcast(bet, A, (float *)(smem + L.oW), (double *)(smem + L.oP));
                const double u = draw_u((unsigned)nx[0], (unsigned)nx[1]);
                a = __popcll(ballot(l < A && cp < u));  // lower_bound
            }
            if (l == 0) {
                if (MZ_STAMPS) sXl[3] = (long long)(__builtin_amdgcn_s_memtime() - ts[0]);  // this wave's end
                draw_slot_set(sXi, (int)(0x80000000u | (unsigned)a));
            }
            wait_lds();
        }
    };

    auto wave1 = [&]() {
        // ======== wave 1: CTree::back_propagate (cnode.cpp:415-450) over the chain ========
        const int P = P_of(), Dp = Dp_of(P);
        TreeHdr *hp;
        int8v hv;  // cursor, tot, D, err, mm_min, mm_max, mm_cnt, leaf
        int r_i, v_i, g_i = apk;  // (!kEntry: apk is the discount)
        // The chain's records, lane i = node i: the arena base in a scalar pair plus a 32-bit byte
        // offset per lane, the arrays' offsets from the packed argument (no round-up, no 64-bit
        // address arithmetic in front of the loads)
        unsigned rA = 0, rC = 0, rPP = 0, rLp = 0;  // A[nb], C[nb], PP[nb], lp[0]
        const size_t nb = (size_t)t * P;            // (!kEntry)
        const float *lpt = nullptr;                 // (!kEntry)
        if constexpr (kEntry) {
            const gchar *hb = hb_of();
            hp = hdr_of(hb);
            hv = sload8<kHdr8>(hb);
            r_i = sload1(in_t(reward)), v_i = sload1(in_t(value));
            g_i = sload1<kIo + (int)(offsetof(ChainIO, k) + offsetof(ChainK, discount))>(ka);
            const unsigned oA8 = oA8_of(), c8 = c8_of(), nbu = (unsigned)t * (unsigned)P;
            rA = oA8 + nbu * 16, rC = rA + kNodeSpanC * c8;
            rPP = oA8 + kNodeSpanPP * c8 + nbu * 4;
            rLp = arena_lp((unsigned)bak & 0xffffffu) << 8;
        } else {
            hp = d.hdr() + t;
            hv = sload8(hp);
            r_i = sload1(reward + t), v_i = sload1(value + t);
            arena();
            lpt = d.lp();
        }
        const gchar *ab = d.base;
        int4 a4[NCH];
        float2 cw[NCH];
        float pp[NCH], lpv[NCH];
        auto load = [&](int D) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                if constexpr (kEntry) {
                    // (lanes past the leaf load the leaf's records: in bounds and never read, where a
                    // test would put an exec mask and eight register clears in front of the loads)
                    const unsigned i = (unsigned)(c * kWave + l), ic = i < (unsigned)D ? i : (unsigned)D;
                    a4[c] = *(const int4 *)(ab + (rA + ic * 16));
                    cw[c] = *(const float2 *)(ab + (rC + ic * 16));
                    pp[c] = *(const float *)(ab + (rPP + ic * 4));
                    lpv[c] = *(const float *)(ab + (rLp + ((unsigned)D - ic) * 4));  // lambda^(D - i): this back-propagation's depth at node i
                } else {
                    const int i = c * kWave + l;
                    a4[c] = make_int4(0, 0, 0, 0);
                    cw[c] = make_float2(0.f, 0.f);
                    pp[c] = 0.f;
                    lpv[c] = 0.f;
                    if (i <= D) {
                        a4[c] = d.A()[nb + i];
                        cw[c] = *(const float2 *)&d.C()[nb + i];
                        pp[c] = d.PP()[nb + i];
                        lpv[c] = lpt[D - i];
                    }
                }
            }
        };
        load(Dp);  // (one round: every address follows from the preloaded arguments)
        if constexpr (kEntry) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(hv), "+s"(r_i), "+s"(v_i), "+s"(g_i)::"memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(hv), "+s"(r_i), "+s"(v_i)::"memory");
        if constexpr (kHand) start_barrier();  // (every wave, before any return: wave 0's slot clear)
        const float r_in = i2f(r_i), v_in = i2f(v_i);
        const int herr = hv[3], D = hv[2], toth = hv[1], leafh = hv[7];
        if (herr) return;  // (wave 0 reports; no wave takes the barrier on the error paths)
        if (D != Dp || toth != D + 1 || leafh != D) {
            if (no_chain(D, P, toth, leafh)) return;  // (wave 0 reports)
            load(D);  // a graph replayed out of sequence: the header's chain
        }
        if constexpr (kEntry) {  // (the whole record in one 16-byte load: its third word is not read)
#pragma unroll
            for (int c = 0; c < NCH; ++c) asm volatile("" : : "v"(a4[c].z));
        }
        const float g = i2f(g_i);
        // the chain's rewards, reversed: sRv[j] = r_{D-j} (r_D = this simulation's reward)
        float rw[NCH];  // (the leaf's reward is this simulation's)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int i = c * kWave + l;
            rw[c] = (i == D) ? r_in : i2f(a4[c].w);
            if (i >= 1 && i <= D) sRv[D - i] = rw[c];
        }
        // What the node updates need and the recurrence does not feed, here, in the shadow of the
        // record loads and of the staging round trip, not behind the recurrence on the launch's
        // chain: the records' store offsets, the LDS offsets of sA / sPP / the lane's key, visit + 1,
        // the total weight, and i - 1 (one unsigned compare with D is then the lane's "node 1..D").
        // Pinned with empty asm: the compiler would sink each to its use.
        // (LDS addresses as 32-bit values: a pinned generic pointer would make the accesses flat.  The
        // new record is pinned whole, visit + 1, the structure word and the reward in place around the
        // value's register: no copy in front of the 16-byte stores.)
        auto lds_of = [&](const void *p) { return (unsigned)(uintptr_t)(lds_void *)p; };
        unsigned stA[NCH], stC[NCH], pSA[NCH], pSP[NCH], pKey[NCH], im1[NCH];
        int4v na[NCH];
        float tw[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const unsigned i = (unsigned)(c * kWave + l);
            stA[c] = rA + i * 16, stC[c] = rC + i * 16;  // (kEntry)
            pSA[c] = lds_of(sA + i), pSP[c] = lds_of(sPP + i);
            pKey[c] = lds_of(sBv) + ((unsigned)D - 1u - i) * 4;  // sBv[D - 1 - i]
            im1[c] = i - 1u;
            na[c] = int4v{a4[c].x + 1, a4[c].y, 0, f2i(rw[c])};
            tw[c] = cw[c].y + lpv[c];
            asm volatile("" : "+v"(stA[c]), "+v"(stC[c]), "+v"(pSA[c]), "+v"(pSP[c]), "+v"(pKey[c]), "+v"(im1[c]),
                         "+v"(na[c]), "+v"(tw[c]));
        }
        // the reductions' identities (lanes past the chain keep them) and lane 63's two store addresses
        float mn = INFINITY, mx = -INFINITY;
        unsigned pX = lds_of(sX), stH = ((unsigned)t << 8) + (unsigned)(kHdr8 + (int)offsetof(TreeHdr, mm_min));  // (kEntry)
        asm volatile("" : "+v"(mn), "+v"(mx), "+v"(pX), "+v"(stH));
        wait_lds();
        stamp(ts, 1);
        // b_{D-1-j} = r_{D-j} + discount * b_{D-j}, j = 0 .. D-1, sixteen levels per LDS round
        // (the next sixteen rewards are read while these run; levels past the root compute values
        // nobody reads: sRv / sBv are padded)
        {
            float b = v_in;
            float4 n0 = *(const float4 *)(sRv), n1 = *(const float4 *)(sRv + 4), n2 = *(const float4 *)(sRv + 8),
                   n3 = *(const float4 *)(sRv + 12);
            for (int j0 = 0; j0 < D; j0 += 16) {
                const float4 c0 = n0, c1 = n1, c2 = n2, c3 = n3;
                n0 = *(const float4 *)(sRv + j0 + 16);
                n1 = *(const float4 *)(sRv + j0 + 20);
                n2 = *(const float4 *)(sRv + j0 + 24);
                n3 = *(const float4 *)(sRv + j0 + 28);
                float4 o0, o1, o2, o3;
                b = c0.x + g * b; o0.x = b;
                b = c0.y + g * b; o0.y = b;
                b = c0.z + g * b; o0.z = b;
                b = c0.w + g * b; o0.w = b;
                b = c1.x + g * b; o1.x = b;
                b = c1.y + g * b; o1.y = b;
                b = c1.z + g * b; o1.z = b;
                b = c1.w + g * b; o1.w = b;
                b = c2.x + g * b; o2.x = b;
                b = c2.y + g * b; o2.y = b;
                b = c2.z + g * b; o2.z = b;
                b = c2.w + g * b; o2.w = b;
                b = c3.x + g * b; o3.x = b;
                b = c3.y + g * b; o3.y = b;
                b = c3.z + g * b; o3.z = b;
                b = c3.w + g * b; o3.w = b;
                *(float4 *)(sBv + j0) = o0;
                *(float4 *)(sBv + j0 + 4) = o1;
                *(float4 *)(sBv + j0 + 8) = o2;
                *(float4 *)(sBv + j0 + 12) = o3;
            }
        }
        wait_lds();
        stamp(ts, 2);
        // ---- every node of the chain, lane i = node i: visits, value set (an append to an empty
        // depth class, utils.cpp:36-44), value (cnode.cpp:42-56); min / max over the q of 1..D ----
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int i = c * kWave + l;
            if (i <= D) {
                // (the read is unconditional -- the leaf's lane reads the word in front of sBv -- so
                // that the key is one select, not a branch around the read)
                const float kb = *(const lds_f32 *)(uintptr_t)pKey[c];
                const float key = (i == D) ? v_in : kb;
                const float ws = cw[c].x + lpv[c] * key;
                const float val = ws / tw[c];
                na[c][2] = f2i(val);
                if constexpr (kEntry) {
                    *(g_int4v *)(d.base + stA[c]) = na[c];
                    *(g_float2v *)(d.base + stC[c]) = float2v{ws, tw[c]};
                } else {
                    d.A()[nb + i] = make_int4(na[c][0], na[c][1], na[c][2], na[c][3]);
                    *(float2 *)&d.C()[nb + i] = make_float2(ws, tw[c]);
                }
                *(lds_int4v *)(uintptr_t)pSA[c] = na[c];  // sA[i]
                *(lds_f32 *)(uintptr_t)pSP[c] = pp[c];    // sPP[i]
                if (im1[c] < (unsigned)D) {               // node 1..D
                    const float q = (rw[c] + g * val) - pp[c];  // get_qsa - father->pred_value
                    mn = fminf(mn, q);
                    mx = fmaxf(mx, q);
                }
            }
        }
        // both reductions at once; lane 63 holds the two results and stores them itself, the pair
        // in one 8-byte store each to LDS and to the header (no v_readlane, no lane 0)
        wave_minmax_to63(mn, mx);
        if (l == kWave - 1) {
            *(lds_float2v *)(uintptr_t)pX = float2v{mn, mx};  // sX[0], sX[1]
            // (the header's normaliser is this wave's: wave 0 skips the barrier in select_walk's
            // fast case and writes the rest of the header)
            if constexpr (kEntry) *(g_float2v *)(d.base + stH) = float2v{mn, mx};  // mm_min, mm_max
            else *(float2 *)&hp->mm_min = make_float2(mn, mx);
            if (MZ_STAMPS) {
                sXl[0] = (long long)(ts[2] - ts[1]);                         // the recurrence
                sXl[1] = (long long)(__builtin_amdgcn_s_memtime() - ts[2]);  // node updates
                sXl[2] = (long long)(ts[1] - ts[0]);                         // round 1
            }
        }
        // no barrier: this wave's LDS writes are done when it ends, and a wave that has ended no longer
        // counts at s_barrier, so wave 0's barrier (the exact case, the fused readback) completes once
        // this wave has ended.  (With a barrier here this wave sat in it until wave 0 ended -- in the
        // fast case wave 0 takes none -- and the MZ_SPANS build recorded it as the launch's last wave,
        // 0.17 us after wave 0; without it the spans period is 3.20 -> 2.98 us, but the product's
        // launch is unchanged, 3.10 us: wave 0 ends last either way, profiles/round6/ab)
        wait_lds();
        span_end(hsx, 1);
    };

    auto wave2 = [&]() {
        // ======== wave 2: the leaf-row gather and the counters ========
        // Straight-line code in issue order (the row class ROW is a template argument): every wait
        // the compiler places then counts exactly the loads issued after the one it needs.
        // The row of this launch's leaf (hidden_state_index_x = hsx) is issued first, from preloaded
        // arguments and src_slot's own scalar load (ROW 1, 2); then one scalar round trip: the outputs' kernel arguments, the
        // header, the handle's constants.  This wave takes no barrier: nothing it does is read by
        // another wave, and s_barrier waits only for the workgroup's waves that have not ended.
        const long long o = (long long)l * 16;
        unsigned char *sbig = smem + L.total;  // (ROW 2: 16 KiB past the layout)
        int4 gv0 = make_int4(0, 0, 0, 0), gv1 = gv0, gv2 = gv0, gv3 = gv0;
        if constexpr (ROW == 1 || ROW == 2) {
            const long long rb = (long long)((unsigned)ppk >> 20) * 16, lst = rb - 16;
            const char *srow = (const char *)(const gchar *)src_slot + (long long)t * rb;
            if constexpr (ROW == 1) {  // up to 4 KiB: four 16-byte registers per lane, offsets clamped into the row
                gv0 = *(const int4 *)(srow + (o < lst ? o : lst));
                gv1 = *(const int4 *)(srow + (o + 1024 < lst ? o + 1024 : lst));
                gv2 = *(const int4 *)(srow + (o + 2048 < lst ? o + 2048 : lst));
                gv3 = *(const int4 *)(srow + (o + 3072 < lst ? o + 3072 : lst));
            } else {  // up to 16 KiB: sixteen LDS-DMA chunks of 1 KiB
#pragma unroll
                for (int k = 0; k < 16; ++k) glds16a(srow + (o + 1024 * k < lst ? o + 1024 * k : lst), sbig + 1024 * k);
            }
        }
        // cursor, tot, D, err, mm_min, mm_max, mm_cnt, leaf, tame, root_vis, leaf_y, hot_tag
        int16v hv = kEntry ? sload16<kHdr8>(hb_of()) : sload16(d.hdr() + t);
        // pool, pool_stride, row_bytes, gather_out, one_minus_rho, o_stats (wave 2's argument line)
        int16v io8 = kEntry ? sload16<kIo>(ka) : sload16((const void *)iop);
        // (every wave takes the start barrier before any return: wave 0's slot clear.  Here ahead of
        // the wait: this wave's round 1 is two dependent scalar round trips with ROW 1, 2, and the
        // other waves would wait at the barrier for the second)
        if constexpr (kHand) start_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(io8), "+s"(hv) : : "memory");
        const int omri = io8[8], osti = io8[9];
        const int P = P_of(), PS = PS_of();
        int rv0 = hv[9];
        if (hv[11] != hv[1]) {  // no valid hot copy: the root's record
            if constexpr (kEntry) {
                rv0 = uni(*(const int *)(d.base + (oA8_of() + (unsigned)t * (unsigned)P * 16)));
            } else {
                arena();
                rv0 = uni(d.A()[(size_t)t * P].x);
            }
        }
        stamp(ts, 1);
        // (typed as global memory: flat accesses would count against lgkmcnt too)
        const char *pool = (const char *)(const gchar *)u64_of(io8[0], io8[1]);
        const long long pool_stride = (long long)u64_of(io8[2], io8[3]);
        const long long row_bytes = (long long)u64_of(io8[4], io8[5]);
        char *gather_out = (char *)(gchar *)u64_of(io8[6], io8[7]);
        const int toth = hv[1], D = hv[2], herr = hv[3], leafh = hv[7];
        const int root_vis0 = rv0;
        const float omr = i2f(omri);
        const char *src = pool + (long long)hsx * pool_stride + (long long)t * row_bytes;  // (ROW 0)
        d.o_stats = (unsigned)osti;
        long long *st = d.stats() + (size_t)t * MZ_S_COUNT;
        const long long st_old = st[l < MZ_S_CYC_HEADER ? l : 0];
        // a dead or inconsistent tree: wave 0 reports; no wave takes the barrier on these paths (all
        // three read the same header)
        if (herr || no_chain(D, P, toth, leafh)) {
            wait_vm();  // (no LDS-DMA may land after the workgroup ends)
            return;
        }
        const int c = D + 1, Ds = c;
        int err = (c + 1 > P) ? kErrPool : 0;
        if (value_lim(1, omr) != 1) err |= kErrValueSet;
        if (SEL && Ds + 1 > PS) err |= kErrPath;
        if (SEL && !err && root_vis0 >= PS) err |= kErrTable;  // the root's child visits index the pUCT table
        stamp(ts, 2);
        stamp(ts, 3);
        stamp(ts, 4);
        if (SEL && ROW != 3 && !err) {
            char *dst = gather_out + (long long)t * row_bytes;
            if constexpr (ROW == 1) {
                // written through (sc0 sc1): the rows are most of this launch's stores, and lines
                // left dirty in L2 are written back at the kernel boundary (same-box A/B: 3m env
                // step 0.4743 -> 0.4679 ms, 2s3z 1.110 -> 1.080; k_tree's 3m row measured 0.5 %
                // slower this way)
                if (o < row_bytes) st_wt16(dst + o, gv0);
                if (o + 1024 < row_bytes) st_wt16(dst + o + 1024, gv1);
                if (o + 2048 < row_bytes) st_wt16(dst + o + 2048, gv2);
                if (o + 3072 < row_bytes) st_wt16(dst + o + 3072, gv3);
            } else if constexpr (ROW == 2) {
                wait_vm();
                // (written through as well: 27m's 13.5 KiB rows, env step 26.42 -> 24.53 ms)
                for (long long o2 = o; o2 < row_bytes; o2 += 16 * kWave) st_wt16(dst + o2, *(const int4 *)(sbig + o2));
            } else {  // any other row: 16-byte copies when aligned, else 4-byte
                if (((row_bytes | pool_stride | (long long)(uintptr_t)pool | (long long)(uintptr_t)gather_out) & 15) == 0) {
                    for (long long o2 = o; o2 < row_bytes; o2 += 16 * kWave) *(int4 *)(dst + o2) = *(const int4 *)(src + o2);
                } else {
                    for (long long o2 = (long long)l * 4; o2 < row_bytes; o2 += 4 * kWave)
                        *(int *)(dst + o2) = *(const int *)(src + o2);
                }
            }
        }
        stamp(ts, 5);
        if (MZ_STAMPS && l == 0) {  // (wave 2's phases, stamped builds: slots wave 0 leaves alone)
            st[MZ_S_CYC_STAGE1] += (long long)(ts[1] - ts[0]);  // scalar round trip
            st[MZ_S_CYC_STAGE2] += (long long)(ts[2] - ts[0]);  // header checks done
            st[MZ_S_CYC_GATHER] += (long long)(ts[4] - ts[0]);  // (the same point: no barrier)
            st[MZ_S_CYC_W1_STAGE2] += (long long)(ts[5] - ts[0]);  // row stored
        }
        if (l < MZ_S_CYC_HEADER) {
            long long add = 0;
            switch (l) {
                case MZ_S_SELECTS: add = SEL ? 1 : 0; break;
                case MZ_S_PATH_EDGES: add = SEL ? Ds : 0; break;
                case MZ_S_SCORED: add = SEL ? Ds : 0; break;
                case MZ_S_EXPANDS: add = 1; break;
                case MZ_S_NEW_CHILDREN: add = 1; break;
                case MZ_S_BACKUP_NODES: add = D + 1; break;
                case MZ_S_MINMAX_NODES: add = D; break;
                default: break;
            }
            st[l] = st_old + add;
        }
        if constexpr (ROW == 2) wait_vm();
        span_end(hsx, 2);
    };

    // The role tests.  Wave 2 first: with a row to gather its round 1 is two dependent round trips
    // (src_slot, then the row's loads, issued ahead of the start barrier), so it is the last wave at
    // the barrier and the other three wait there for it.  Then the waves of the two arms, the
    // back-propagation and the draw; wave 0 falls through.
    if constexpr (kEntry) {
        if (__builtin_expect_with_probability(role(2), 0, 0.7)) {
            wave2();
            return;
        }
        if (__builtin_expect_with_probability(role(1), 0, 0.7)) {
            wave1();
            return;
        }
        if (W4 && __builtin_expect_with_probability(role(3), 0, 0.7)) {
            wave3();
            return;
        }
    } else {
        // The common prologue of the earlier entry: what every role derives from the preloaded
        // arguments, computed once ahead of the role tests.  The roles' lambdas name the same
        // expressions (P_of() and the rest), so the compiler reuses these values there; without the
        // empty asm, which uses them here, it would sink each computation into the roles instead.
        const int P = P_of(), PS = PS_of(), A = A_of(), Dp = Dp_of(P);
        const size_t nb = (size_t)t * P;
        TreeHdr *hp = d.hdr() + t;
        asm volatile("" : : "s"(P), "s"(PS), "s"(A), "s"(Dp), "s"(nb), "s"(hp));
        if (W4 && wv == 3) {
            wave3();
            return;
        }
        if (wv == 1) {
            wave1();
            return;
        }
        if (wv == 2) {
            wave2();
            return;
        }
    }

    // ======== wave 0: CTree::expand (cnode.cpp:224-295) of the leaf: one draw ========
    const int A = A_of();
    const int P = P_of(), PS = PS_of(), Dp = Dp_of(P), fast_ok = (int)((unsigned)bak >> 31);
    const size_t nb = (size_t)t * P;
    TreeHdr *hp;
    // cursor, tot, D, err, mm_min, mm_max, mm_cnt, leaf, tame, root_vis, leaf_y, hot_tag, nxt[0 .. 3]
    int16v hv;
    // idx_x, idy, act and the handle's constants (wave 0's argument line: ChainIO, ChainK)
    int16v kv;
    int r_i, v_i;
    float pol, bet;
    if constexpr (kEntry) {
        const gchar *hb = hb_of();
        hp = hdr_of(hb);
        hv = sload16<kHdr8>(hb);
        kv = sload16<kIo + (int)offsetof(ChainIO, idx_x)>(ka);
        r_i = sload1(in_t(reward)), v_i = sload1(in_t(value));
        pol = in_row(policy, A), bet = in_row(beta, A);
    } else {
        hp = d.hdr() + t;
        hv = sload16(hp);
        kv = sload16((const char *)iop + offsetof(ChainIO, idx_x));
        r_i = sload1(reward + t), v_i = sload1(value + t);
        pol = policy[(size_t)t * A + (l < A ? l : 0)];
        bet = beta[(size_t)t * A + (l < A ? l : 0)];
    }
    if constexpr (kHand) {  // the hand-over slot, cleared ahead of the start barrier (round 1's wait covers the store)
        if (l == 0) draw_slot_set(sXi, 0);
    }
    // This launch's record stores, one per lane, from addresses held in registers: lane 0 the child's
    // C, lane 1 the leaf's Bn, lane 2 the child's A, lane 3 the child's Bn (16 bytes each), and the
    // dwords of lane 0 the child's PP, lanes 1-3 idx_x / idy / act.  The node addresses follow from
    // the preloaded arguments (the leaf of an in-sequence launch is hsx): computed here, while round
    // 1's loads are in flight, in vector registers (the scalar file is full).
    const uintptr_t abase = (uintptr_t)d.base;
    uintptr_t p16, p4;
    if constexpr (kEntry) {
        arena_nodes_at(d, (unsigned)apk & 0xffffu, (unsigned)apk >> 16);  // (for the reads off the in-sequence path)
        const unsigned oA8 = oA8_of(), c8 = c8_of();
        const unsigned k16 = (l == 0) ? kNodeSpanC : (l == 2) ? 0u : kNodeSpanBn;  // the lane's array, in units of c
        const unsigned nd = (unsigned)t * (unsigned)P + (unsigned)Dp;
        p16 = abase + (oA8 + k16 * c8 + (nd + (l == 1 ? 0u : 1u)) * 16);
        p4 = abase + (oA8 + kNodeSpanPP * c8 + (nd + 1) * 4);
    } else {
        arena();
        unsigned oA = d.o_A, oBn = d.o_Bn, oC = d.o_C;
        asm volatile("" : "+s"(oA), "+s"(oBn), "+s"(oC));  // (values, not fields: no table in scratch)
        const unsigned o16 = (l == 0) ? oC : (l == 2) ? oA : oBn;
        p16 = abase + (size_t)o16 * 256 + (nb + (size_t)Dp + (l == 1 ? 0 : 1)) * 16;
        p4 = abase + (size_t)d.o_PP * 256 + (nb + (size_t)Dp + 1) * 4;
    }
    asm volatile("" : "+v"(p16), "+v"(p4));
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+s"(hv), "+s"(kv), "+s"(r_i), "+s"(v_i)
                 :
                 : "memory");
    if constexpr (kHand) start_barrier();  // (every wave, before any return: the slot is clear from here)
    // The root's visit count and the leaf's Bn.y: the header's copy when the previous launch left a
    // valid one (k_prepare, k_chain3), else the records (one more round trip: the first fused launch
    // after a host-path step, or after any other kernel wrote the header)
    int root_vis0 = hv[9], leaf_by = hv[10];
    if (hv[11] != hv[1]) {
        root_vis0 = uni(d.A()[nb].x);
        leaf_by = uni(d.Bn()[nb + Dp].y);
    }
    // The next expansion's engine words (the header's nxt), read now for select_walk's fast case --
    // one word per level below the root (its first level is forced while it has one visit): they
    // land while the distribution is built.  The exact case re-reads them after the barrier.
    constexpr int kK0 = (int)((offsetof(ChainIO, k) - offsetof(ChainIO, idx_x)) / 4);  // ChainK's first dword in kv
    static_assert(kK0 == 6 && offsetof(ChainK, o_sq) == 32 && offsetof(ChainK, discount) == 36, "wave 0's argument line");
    const int omri = kv[kK0], gW = kv[kK0 + 1];
    d.o_R = (unsigned)kv[kK0 + 2];
    d.o_err = (unsigned)kv[kK0 + 3];
    d.o_D = (unsigned)kv[kK0 + 4];
    d.o_stats = (unsigned)kv[kK0 + 5];
    const float gdelta = i2f(kv[kK0 + 6]);
    d.o_pb = (unsigned)kv[kK0 + 7];
    d.o_sq = (unsigned)kv[kK0 + 8];
    const float discount = i2f(kEntry ? kv[kK0 + 9] : apk);
    const unsigned *Rt = d.R() + (size_t)t * gW;
    const int dA = (A >= 2) ? 2 : 0;
    const int words_fast = SEL ? (hv[2] + 1) - ((root_vis0 + 1 <= 1) ? 1 : 0) : 0;
    const int wi = hv[0] + dA + words_fast + l;
    const unsigned w_fast = Rt[(wi >= 0 && wi < gW) ? wi : 0];
    const float r_in = i2f(r_i), v_in = i2f(v_i);
    int *const idx_x = (int *)(gchar *)u64_of(kv[0], kv[1]), *const idy = (int *)(gchar *)u64_of(kv[2], kv[3]);
    int *const act = (int *)(gchar *)u64_of(kv[4], kv[5]);
    TreeHdr h;
    h.cursor = hv[0];
    h.tot = hv[1];
    h.D = hv[2];
    h.err = hv[3];
    h.leaf = hv[7];
    h.tame = hv[8];
    h.nxt[0] = (unsigned)hv[12];
    h.nxt[1] = (unsigned)hv[13];
    if (h.err) {  // a dead tree stays dead and re-reports its error
        if (l == 0) {
            if (SEL) {
                idx_x[t] = 0;
                idy[t] = t;
                act[t] = 0;
            }
            atomicOr(d.err(), h.err);
        }
        return;
    }
    const int D = h.D;
    if (D != Dp || h.tot != D + 1 || h.leaf != D) {
        if (no_chain(D, P, h.tot, h.leaf)) {  // refuse
            if (l == 0) {
                if (SEL) {
                    idx_x[t] = 0;
                    idy[t] = t;
                    act[t] = 0;
                }
                hp->err = kErrPath;
                atomicOr(d.err(), kErrPath);
            }
            return;
        }
        // out of sequence: the header's leaf (waited for here: no wait for it on the path in sequence)
        leaf_by = uni(d.Bn()[nb + D].y);
        p16 += (long long)(D - Dp) * 16;
        p4 += (long long)(D - Dp) * 4;
    }
    stamp(ts, 1);
    const int leaf = D, c = D + 1;  // the new child
    int cursor = h.cursor;
    int a = 0;
    const float bh = 1.0f;  // betahat_prob = count / sampled_times = 1 / 1
    // ---- everything the draw does not feed, before the draw ----
    // The errors but kErrTable's bit: the records are created unless err1, the outputs report a
    // selection unless any error -- and whether there is one is known here (kErrTable depends on the
    // draw only when another error is set already).
    const float omr = i2f(omri);
    const int Ds = c;
    int err1 = (c + 1 > P) ? kErrPool : 0;
    if (value_lim(1, omr) != 1) err1 |= kErrValueSet;  // (count 1: size_lim must be 1, utils.cpp:31)
    int errp = err1;
    if (SEL && Ds + 1 > PS) errp |= kErrPath;
    // the root's total child visits after this back-propagation index the pUCT table (select_walk
    // checks it in the fast case; in the exact case it is the largest parent count of the path)
    const bool tbl = SEL && root_vis0 >= PS;
    const bool any_err = errp != 0 || tbl;
    const bool tame0 = h.tame && tame_val(v_in) && tame_val(r_in);
    const int md = md_of(leaf_by) < 0 ? 0 : md_of(leaf_by);
    // the records' words by lane (above); the drawn words -- lane 2's prior, lane 3's action and
    // act[t] -- are set after the draw
    int leaf_y = pack_y(1, act_of(leaf_by), md), idx_v = any_err ? 0 : hsx;  // (idx_x: the expanded leaf's)
    asm volatile("" : "+s"(leaf_y), "+s"(idx_v));
    int4v d16 = {l == 1 ? c : 0, l == 1 ? leaf_y : 0, l == 1 ? f2i(v_in) : 0, l == 1 ? hsx : (l == 3 ? -1 : 0)};
    int d4 = (l == 0) ? f2i(v_in) : t;
    d4 = (l == 1) ? idx_v : d4;
    uintptr_t xp = (uintptr_t)((l == 1) ? idx_x : (l == 2) ? idy : act) + (size_t)t * 4;
    p4 = (l == 0) ? p4 : xp;
    const bool st16 = l < 2 && !err1, st4 = (l == 0) ? !err1 : (SEL && l < 3);
    // the stores without a drawn word go first: C[gi], Bn[leaf], PP[gi], idx_x, idy
    auto early = [&]() {
        if (st16) st_lane16(p16, d16);
        if (st4) st_lane4(p4, d4);
        asm volatile("" : "+v"(p16), "+v"(p4), "+v"(d16) : : "memory");
    };
    // every lane's prior * betahat_prob / beta_prob (eps = 0 after the root) and whether it is tame:
    // after the draw only the drawn lane's are read
    float prior_l = 0.f;
    int wild_l = 0;
    auto priors = [&]() {
        prior_l = pol * bh / bet;
        wild_l = tame_prior(prior_l) ? 0 : 1;
        asm volatile("" : "+v"(prior_l), "+v"(wild_l));
    };
    int fell = 0;  // (stamped builds: hand-overs that ran out of polls; kDS: launches this wave drew)
    bool ds = false;  // (kDS) the draw wave stores the drawn words: this wave reads no action
    if constexpr (kDS) {
        priors();
        early();
        stamp(ts, 7);
        // (D == hsx in range, so the early stores' addresses above are this predicate's)
        ds = draw_pred(hv, omri, kv[kK0 + 9], r_i, v_i, wild_l != 0);
        if (!ds) {
            // this wave draws itself, in registers, from the same words in the same order
            fell = 1;
            if (A >= 2) {
                const float w = (l < A) ? bet : 0.f;
                const double cp = (A <= 16) ? cdf_short(A, w) : cdf_lane((double)w, A);
                const double u = draw_u(h.nxt[0], h.nxt[1]);
                a = __popcll(ballot(l < A && cp < u));  // lower_bound
            }
        }
        if (A >= 2) cursor += 2;
    } else if constexpr (W4) {
        // the draw wave's action: a bounded poll of the hand-over slot (an LDS read, a readfirstlane
        // and a scalar test each)
        priors();
        early();
        stamp(ts, 7);
        int v = 0;
        for (int i = 0; i < kDrawPolls; ++i) {
            v = uni(draw_slot_get(sXi));
            if (v < 0) break;
        }
        if (v < 0) {
            a = v & 0x7fffffff;
        } else {
            // the bound ran out: this wave draws itself, in registers (sW / sP may still be the draw
            // wave's), from the same words in the same order
            fell = 1;
            if (A >= 2) {
                const float w = (l < A) ? bet : 0.f;
                const double cp = (A <= 16) ? cdf_short(A, w) : cdf_lane((double)w, A);
                const double u = draw_u(h.nxt[0], h.nxt[1]);
                a = __popcll(ballot(l < A && cp < u));  // lower_bound
            }
        }
        if (A >= 2) cursor += 2;
    } else if (A >= 2) {
        // the draw's u, from the header's two engine words
        double u = 0.0;
        const double cp = cdf_bcast(
            bet, A, (float *)(smem + L.oW), (double *)(smem + L.oP),
            [&]() {  // (while the distribution's first LDS store is in flight)
                priors();
                early();
            },
            [&]() {  // (while its second is)
                u = draw_u(h.nxt[0], h.nxt[1]);
                asm volatile("" : "+v"(u));
            });
        a = __popcll(ballot(l < A && cp < u));  // lower_bound
        cursor += 2;
    } else {
        priors();
        early();
    }
    a = uni(a);
    stamp(ts, 2);
    if constexpr (kDS && !MZ_STAMPS) {
        // ---- the draw wave stores the drawn words: the rest of the header and the end ----
        // The predicate gives err == 0, tame == 1 and select_walk's fast case (one word per level but
        // the forced first one; no barrier).  The wait is counted: behind the engine words' load
        // this wave has issued early()'s two stores and nothing else (both run under the predicate:
        // err1 == 0, so lanes 0 and 1 store), and loads and stores retire in issue order -- no wait
        // for the stores' own round trip, which the poll of the hand-over used to cover.
        // (stamped builds take the general path below: wave 1's stamps come through the barrier)
        if (ds) {
            unsigned nxt_ds = (wi >= 0 && wi < gW) ? w_fast : 0u;  // (cursor + words + l == wi)
            asm volatile("s_waitcnt vmcnt(2)" : "+v"(nxt_ds) : : "memory");
            if (l < kNxt) hp->nxt[l] = nxt_ds;
            if (l == 0) {
                hp->cursor = cursor + Ds - ((root_vis0 + 1 <= 1) ? 1 : 0);
                hp->tot = c + 1;
                hp->D = Ds;
                hp->err = 0;
                hp->mm_cnt = D;  // (mm_min / mm_max: wave 1; leaf_y: the draw wave)
                hp->tame = 1;
                hp->leaf = c;
                hp->root_vis = root_vis0 + 1;
                hp->hot_tag = c + 1;
            }
            span_close(hsx, rt0);
            return;
        }
    }
    // ---- after the draw: the drawn lane's prior, the words it feeds, their stores ----
    const float prior = rlf(prior_l, a);
    const bool wild = rl(wild_l, a) != 0;
    const int tame = (tame0 && !wild) ? 1 : 0;
    const bool fast = !SEL || (fast_ok && tame && fabsf(discount) <= 1.0f);  // (no selection: no words)
    int err = errp;
    if (tbl && (fast || !errp)) err |= kErrTable;
    // The fast case's engine words have landed with the stores above (issued a distribution ago):
    // one wait here, before this launch's last stores, instead of the compiler's after them
    unsigned nxt_fast = (wi >= 0 && wi < gW) ? w_fast : 0u;  // (cursor + words + l == wi)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(nxt_fast) : : "memory");
    if (fast && l < kNxt) hp->nxt[l] = nxt_fast;
    // (sel_lane: two v_cndmask; the compiler makes branches of the selects)
    d16.y = f2i(sel_lane(sel_lane(i2f(d16.y), prior, 1ull << 2), i2f(pack_y(0, a, -1)), 1ull << 3));
    // (ds: the draw wave stores the drawn words -- the child's A and Bn, act[t], D[child], leaf_y below)
    if ((l == 2 || l == 3) && !err1 && !ds) st_lane16(p16, d16);
    if (SEL && l == 3 && !ds) st_lane4(p4, any_err ? 0 : a);
    if (!err1 && leaf == 0 && !ds) {  // (readbacks: root children)
        const float pol_a = rlf(pol, a), bet_a = rlf(bet, a);
        if (l == 0) d.D()[nb + c] = make_float4(pol_a, bet_a, bh, 0.f);
    }
    stamp(ts, 3);
    // wave 1's back-propagation (sA, sPP) and min / max: read by the exact case and the fused
    // readback only.  In select_walk's fast case (one word per level) wave 0 takes no barrier (wave
    // 1's waits for this wave's end instead: s_barrier counts the waves that have not ended)
    const bool bar = MZ_STAMPS || !SEL || !fast;  // (stamped builds: wave 1's stamps come through LDS)
    if (bar) lds_barrier();
    stamp(ts, 4);
    const float mn = bar ? unif(sX[0]) : 0.f, mx = bar ? unif(sX[1]) : 0.f;
    const int mm_cnt = D;
    int words = 0;
    if (SEL && fast) {
        words = Ds - ((root_vis0 + 1 <= 1) ? 1 : 0);  // one per level but the forced first one
    } else if (SEL && !err) {
        // ---- select_walk's exact case: every level's tie list must be non-empty to consume a
        // word (score >= FLOAT_MIN, not NaN); levels 1..Ds scored in parallel ----
        sA[c] = make_int4(0, f2i(prior), f2i(0.0f), f2i(0.0f));
        wait_lds();
        const int root_visit = uni(sA[0].x);
        const bool mm_on = mm_cnt > 0;
        float den = 0.f;
        if (mm_on) {
            const float delta = mx - mn;
            den = (gdelta < delta) ? delta : gdelta;  // std::max(delta_lb, delta)
        }
        const float *pbt = d.pb();
        const double *sqt = d.sq();
        for (int i0 = 0; i0 <= Ds; i0 += kWave) {
            const int i = i0 + l;
            bool valid = false;
            if (i >= 1 && i <= Ds && !(i == 1 && root_visit <= 1)) {
                const int n = sA[i - 1].x - 1;  // the parent's total_children_visit_counts (< PS: checked)
                const int4 ca = sA[i];
                const float pp = (i == Ds) ? v_in : sPP[i];
                float vs = (ca.x == 0) ? 0.0f : ((i2f(ca.w) + discount * i2f(ca.z)) - pp);
                if (mm_on) vs = (vs - mn) / den;
                if (vs < 0) vs = 0;
                if (vs > 1) vs = 1;
                const float pbc = (float)((double)pbt[n] * (sqt[n] / (double)(ca.x + 1)));
                const float sc = pbc * i2f(ca.y) + vs;
                valid = sc >= -1000000.0f;  // FLOAT_MIN (utils.h:12)
            }
            words += __popcll(ballot(valid));
        }
    }
    stamp(ts, 5);
    if (!fast && l < kNxt) {  // (the fast case's words: stored above)
        unsigned nxt_w = 0;
        if (SEL && !err && cursor + words + l < gW) nxt_w = Rt[cursor + words + l];
        hp->nxt[l] = nxt_w;
    }
    if (l == 0) {
        hp->cursor = err ? h.cursor : cursor + words;
        hp->tot = err ? h.tot : c + 1;
        hp->D = (err || !SEL) ? h.D : Ds;
        hp->err = err;
        hp->mm_cnt = mm_cnt;  // (mm_min / mm_max: wave 1)
        hp->tame = tame;
        hp->leaf = (err || !SEL) ? h.leaf : c;
        // the hot copy for the next launch: wave 1 adds this back-propagation's visit to the root, and
        // the new leaf is the child created above (its Bn.y as stored there)
        hp->root_vis = root_vis0 + 1;
        if (!ds) hp->leaf_y = pack_y(0, a, -1);
        hp->hot_tag = (err || !SEL) ? 0 : c + 1;
    }
    if constexpr (!SEL) {
        // the fused readback (mz_expand_backup_readback, include/mzdriver.h): the search's outputs
        // from this launch's final records.  Wave 1 left every chain node's new {visit, prior, value,
        // reward} in sA (read after the barrier above); the structure records come from HBM but the
        // leaf's, rewritten above, and the root children's probabilities from HBM (written at prepare)
        // (a tree that failed writes an empty readback -- no children, value 0 -- rather than leave
        // the caller's buffers as they were; the error word reports it)
        const RbDesc *rbd = (const RbDesc *)(const void *)iop->gather_out;
        if (rbd) {
            const int4 rbn = err ? make_int4(0, 0, 0, 0) : uni4(d.Bn()[nb]);
            const int nc = nc_of(rbn.y), fc = rbn.x;
            const int md = md_of(leaf_by) < 0 ? 0 : md_of(leaf_by);
            const int4 leaf_new = make_int4(c, pack_y(1, act_of(leaf_by), md), f2i(v_in), hsx);
            int4 ca = make_int4(0, 0, 0, 0), cb = ca;
            float4 cd = make_float4(0.f, 0.f, 0.f, 0.f);
            if (l < nc) {
                const int n = fc + l;
                ca = sA[n];
                cb = (n == leaf) ? leaf_new : d.Bn()[nb + n];
                cd = d.D()[nb + n];
            }
            readback_emit(rbd->o, rbd->disc, rbd->Wd, t, A, 1, nc, err ? make_int4(0, 0, 0, 0) : sA[0], ca, cb, cd,
                          nullptr);
        }
    }
    stamp(ts, 6);
    if (MZ_STAMPS && l >= MZ_S_CYC_HEADER && l < MZ_S_COUNT) {
        long long *st = d.stats() + (size_t)t * MZ_S_COUNT;
        long long add = 0;
        switch (l) {
            case MZ_S_CYC_HEADER: add = (long long)(ts[1] - ts[0]); break;   // round 1
            case MZ_S_CYC_EXP_CDF: add = (long long)(ts[2] - ts[1]); break;  // distribution + draw
            case MZ_S_CYC_EXPAND: add = (long long)(ts[3] - ts[2]); break;   // child, outputs
            case MZ_S_CYC_BACKUP: add = (long long)(ts[4] - ts[3]); break;   // waiting at the barrier
            case MZ_S_CYC_SELECT: add = (long long)(ts[5] - ts[4]); break;   // selection (exact case)
            case MZ_S_CYC_EPILOGUE: add = (long long)(ts[6] - ts[5]); break; // header
            case MZ_S_CYC_BAK_BOOT: add = sXl[0]; break;                     // wave 1: recurrence
            case MZ_S_CYC_BAK_NODES: add = sXl[1]; break;                    // wave 1: node updates
            case MZ_S_CYC_W1_ROUND1: add = sXl[2]; break;                    // wave 1: round 1
            // the draw wave (W4): its end after launch start, wave 0's wait at the hand-over slot
            // (part of the distribution + draw span above), hand-overs that ran out of polls (a count)
            case MZ_S_CYC_EXP_DRAW: add = (kDS ? ds : W4) ? sXl[3] : 0; break;  // (kDS: stamped when it stored)
            case MZ_S_CYC_BAK_WAIT: add = W4 ? (long long)(ts[2] - ts[7]) : 0; break;
            case MZ_S_CYC_EXP_NODES: add = fell; break;
            case MZ_S_STAMPED: add = 1; break;
            default: break;
        }
        const bool w2_slot = l == MZ_S_CYC_STAGE1 || l == MZ_S_CYC_STAGE2 || l == MZ_S_CYC_GATHER ||
                             l == MZ_S_CYC_W1_STAGE2;
        if (!w2_slot) st[l] += add;
    }
    if (l == 0 && err) atomicOr(d.err(), err);
    span_close(hsx, rt0);
}
