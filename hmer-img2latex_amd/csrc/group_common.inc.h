// Helpers shared by the grouped persistent kernels (decode_group*.inc.h, beam_group.inc.h, train_group.inc.h): seating,
// bounded polls, placement exchange, tagged-granule exchange between the workgroups of a group, greedy ids epilogue,
// phase stamps, DPP reduce-scatter, packed-FMA tiles, arg-max keys.
// Included inside each translation unit's anonymous namespace.
#pragma once
typedef unsigned long long u64_t;
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr long long GRP_TIMEOUT_TICKS = 300000000ll;   // 3 s of the 100 MHz wall clock

// Per-launch options of a grouped kernel.  A group only makes progress while its four workgroups are resident
// together; the launch is not cooperative, so every poll has a wall-clock limit.  Two limits: the FIRST poll of a
// workgroup (the placement exchange: "are my three peers there at all?") gets a short one -- 10 ms plus what earlier
// groups of the same launch may legitimately hold the CUs for (50 us per step) -- so that on a GPU shared with other
// work the launch gives up in milliseconds and the host falls back to the row-per-workgroup kernel; every later poll
// (peers known to be resident) keeps the 3 s limit.  drop_member is a TEST hook (I2L_FLAG_TEST_DROP_MEMBER): member 3
// of every group exits at once, which forces the time-out path end to end.
struct GroupOpts {
    long long limit_first, limit_step;
    int agent_scope;      // != 0: every exchange store at agent scope (I2L_FLAG_AGENT_SCOPE_EXCHANGE)
    int drop_member;
};
inline GroupOpts group_opts(int steps, int flags) {
    GroupOpts o;
    o.limit_first = 1000000ll + 5000ll * (long long)steps;
    o.limit_step = GRP_TIMEOUT_TICKS;
    if (flags & I2L_FLAG_TEST_SHORT_TIMEOUT) o.limit_first = o.limit_step = 200000ll;      // 2 ms
    o.agent_scope = (flags & I2L_FLAG_AGENT_SCOPE_EXCHANGE) ? 1 : 0;
    o.drop_member = (flags & I2L_FLAG_TEST_DROP_MEMBER) ? 1 : 0;
    return o;
}
// status block of a grouped launch (zeroed by the launch's memset node): [0] != 0 a poll timed out, [1] groups that
// went through the placement exchange, [2] of those, groups whose four members measured ONE XCD (L2-local stores)
constexpr int GRP_STAT_FAILED = 0, GRP_STAT_GROUPS = 1, GRP_STAT_LOCAL = 2;

// Residency signal of a grouped launch (i2l_greedy_decode_ex's resident_flag / resident_value): member 0 of every group
// counts its group in status[GRP_STAT_GROUPS] once all members have answered the placement exchange, i.e. ARE RESIDENT; the
// group that completes the count publishes resident_value at agent scope.  A stream that must not start before this
// launch owns its CUs waits for the word (i2l_stream_wait_value32) -- a dependency, where r03 guessed with a 30 us delay.
// The word is a wrapping sequence that several launches may share (decode streams > 1): publish_max32 only moves it FORWARD,
// so a launch that assembles after a later one cannot take the word back and leave a waiter sitting out its time-out.
__device__ __forceinline__ void publish_max32(unsigned* flag, unsigned value) {
    unsigned old = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while ((int)(value - old) > 0 &&
           !__hip_atomic_compare_exchange_strong(flag, &old, value, __ATOMIC_RELEASE, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT)) {
    }
}
__device__ __forceinline__ void count_resident_group(unsigned* status, int n_groups, unsigned* flag, unsigned value) {
    const unsigned before = atomicAdd(status + GRP_STAT_GROUPS, 1u);
    if (flag && before + 1u == (unsigned)n_groups) publish_max32(flag, value);
}


// Seating of a grouped launch with Q members per group: the grid is cut into slices of 8 Q workgroups, and slice a holds
// groups 8a .. 8a + 7; member m of group 8a + x is workgroup 8Qa + x + 8m.
// Progress: a group's members are 8 block ids apart -- one XCD under round-robin placement (speed only) -- and workgroups
// are dispatched in index order, so on a GPU with at least the 8Q CUs of one grid slice free some complete group is
// resident and runs to its end, freeing its CUs for the next.  That is an assumption about the dispatcher and about what
// else runs on the device, not something HIP promises (the launch is not cooperative): with fewer CUs free every resident
// workgroup may be waiting for a member that is not, so EVERY poll is bounded by a wall-clock limit (PollClock): on expiry
// the workgroup raises status[0], marks its outputs as failed and exits, its peers follow by their own limits, and the
// host wrapper reports the failure and re-runs on the row-per-workgroup kernel; the GPU is never left spinning.
struct GroupSeat {
    int group, m;
};
template <int Q>
__device__ __forceinline__ GroupSeat group_seat() {
    static_assert(Q == 4 || Q == 8 || Q == 16, "members per group");
    const int within = blockIdx.x & (8 * Q - 1);
    return {(int)(blockIdx.x / (8 * Q)) * 8 + (within & 7), within >> 3};
}
// workgroups of a launch of n_groups groups with q members (whole slices; the surplus workgroups return at once)
__host__ __device__ constexpr int group_grid(int n_groups, int q) { return (n_groups + 7) / 8 * 8 * q; }
// exchange bytes of such a launch: one region per group of the grid
constexpr size_t group_xchg_bytes(int n_groups, size_t per_group) { return (size_t)group_grid(n_groups, 1) * per_group; }

// Wall clock of one bounded poll: every call sleeps once; every 256th call reads the 100 MHz clock, the first reading
// starts the limit and expired() reports true once `limit` ticks have passed since then.
struct PollClock {
    long long t_start = 0;
    unsigned spins = 0;
    __device__ __forceinline__ bool expired(long long limit) {
        __builtin_amdgcn_s_sleep(1);
        if ((++spins & 255u) != 0) return false;
        const long long now = (long long)wall_clock64();
        if (t_start == 0) { t_start = now; return false; }
        return now - t_start > limit;
    }
};

// local == false: sc1 store (write-through to memory, seen from every XCD).  local == true (all four members were
// found on ONE XCD): sc0 store, the line stays in that XCD's L2 where the peers' sc1 loads (L1 bypassed) find it --
// an L2 round trip instead of a memory one.
// The L2-local flavour rests on gfx950's write-through L1 (a workgroup-scope store still reaches the XCD's L2, where the
// peers' L1-bypassing polls find it), NOT on the HSA memory model: it is compiled for gfx950 only; any other target gets
// the conformant agent-scope store whatever the caller measured.
__device__ __forceinline__ void store_granule(u64_t* g, u64_t v, bool local) {
#if defined(__gfx950__)
    if (local) { __hip_atomic_store(g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); return; }
#endif
    __hip_atomic_store(g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64_t granule(unsigned tag, float v) { return ((u64_t)tag << 32) | (u64_t)__float_as_uint(v); }
__device__ __forceinline__ u64_t load_granule(const u64_t* g) {
    return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Placement exchange, run by the 64 lanes of wave 0: are the Q members on one XCD?  Each publishes its XCC id in the
// granule at xg[m * gran + xslot] (sc1, seen from anywhere) and polls its Q - 1 peers' under limit_first.  Measured,
// never assumed: equal ids let the caller switch the granule stores to the L2-local flavour, and correctness does not
// depend on it (a member that times out here fails the launch like any other poll).  drop_member (test hook): member 3
// stays silent, its peers time out.  No LDS, no barrier: the caller's other waves may work meanwhile.
struct Placement {
    bool timed_out, one_xcd;
};
template <int Q>
__device__ __forceinline__ Placement group_placement(u64_t* xg, int gran, int xslot, int m, const GroupOpts& o) {
    const int lane = threadIdx.x & 63;
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 0xFu;
    if (lane == 0 && !(o.drop_member && m == 3))
        store_granule(xg + (size_t)m * gran + xslot, granule(0xC0DEu, __uint_as_float(xcc)), false);
    const int pq = (lane & (Q - 1)) + ((lane & (Q - 1)) >= m ? 1 : 0);
    u64_t pv = 0;
    bool bad = false;
    PollClock clk;
    for (;;) {
        bool ok = true;
        if (lane < Q - 1) { pv = load_granule(xg + (size_t)pq * gran + xslot); ok = (unsigned)(pv >> 32) == 0xC0DEu; }
        if (__all(ok)) break;
        if (clk.expired(o.limit_first)) { bad = true; break; }
    }
    return {bad, __all(lane >= Q - 1 || (unsigned)pv == xcc) != 0};
}
// Placement statistics of a greedy decode launch, reported by member 0 once its peers answered: the group counts as
// resident (residency signal) and, when its members share one XCD and the stores are L2-local, in GRP_STAT_LOCAL.
// Beam search and training do not count.
__device__ __forceinline__ void report_group(unsigned* status, int n_groups, unsigned* flag, unsigned value, bool local) {
    count_resident_group(status, n_groups, flag, value);
    if (local) atomicAdd(status + GRP_STAT_LOCAL, 1u);
}

// Greedy decode epilogue of a workgroup of NT threads: after a failure status[0] is raised, the row's ids are -3
// (checked by the host wrappers) and the lane's logits, if any (lrow[t * lstride]), NaN; otherwise the steps from t on,
// never executed (sticky stop), get -1.
template <int NT>
__device__ __forceinline__ void greedy_finish(int32_t* ids_row, bool failed, int t, int T, unsigned* status,
                                              float* lrow = nullptr, int lstride = 0) {
    const int tid = threadIdx.x;
    if (failed) {
        if ((tid & 63) == 0) atomicOr(status, 1u);
        if (ids_row) for (int tt = tid; tt < T; tt += NT) ids_row[tt] = -3;
        if (lrow) for (int tt = 0; tt < T; ++tt) lrow[(size_t)tt * lstride] = __builtin_nanf("");
    } else if (ids_row) {
        for (int tt = t + tid; tt < T; tt += NT) ids_row[tt] = -1;
    }
}

// Phase stamps (profiling build, -DI2L_GROUP_STAMPS): I2L_STAMP(i) adds the wall-clock ticks since the previous stamp
// to st_.acc[i]; each kernel reads st_.acc out into status[8 + ...] in its own layout (profiles/*stamps*).
#ifdef I2L_GROUP_STAMPS
struct StampAcc {
    long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long last = (long long)wall_clock64();
    __device__ __forceinline__ void operator()(int i) {
        const long long n = (long long)wall_clock64();
        acc[i] += n - last;
        last = n;
    }
};
#define I2L_STAMPS_BEGIN StampAcc st_
#define I2L_STAMP(i) st_(i)
#else
#define I2L_STAMPS_BEGIN do { } while (0)
#define I2L_STAMP(i) do { } while (0)
#endif

// DPP controls: quad_perm [1,0,3,2] (lane ^ 1), quad_perm [2,3,0,1] (lane ^ 2), row_half_mirror (lane -> 7 - lane
// within 8), row_ror:n (rotate within 16), row_shl:n (lane reads lane + n)
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HMIRROR = 0x141, DPP_ROR4 = 0x124, DPP_ROR8 = 0x128,
              DPP_SHL4 = 0x104, DPP_SHL8 = 0x108;
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
// One level of a reduce-scatter between a lane and its DPP partner: the pair holds partial sums of the same two
// values (a, b); the lane with sel == false keeps a, its partner keeps b, each adds the other's partial.
template <int CTRL>
__device__ __forceinline__ float rs_level(float a, float b, bool sel) {
    const float keep = sel ? b : a, send = sel ? a : b;
    return keep + dpp_f<CTRL>(send);
}
__device__ __forceinline__ f32x2 splat2(float x) { return f32x2{x, x}; }
// (value, index) as one unsigned 64-bit key whose order is "larger value first, then smaller index": arg max with
// first-index ties becomes a branch-free integer max
__device__ __forceinline__ u64_t am_key(float v, int i) {
    unsigned u = __float_as_uint(v + 0.0f);                 // -0 -> +0
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return ((u64_t)u << 32) | (u64_t)(0xFFFFFFFFu - (unsigned)i);
}
__device__ __forceinline__ float am_val(u64_t k) {
    unsigned u = (unsigned)(k >> 32);
    u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
    return __uint_as_float(u);
}
__device__ __forceinline__ int am_idx(u64_t k) { return (int)(0xFFFFFFFFu - (unsigned)k); }
__device__ __forceinline__ u64_t umax64(u64_t a, u64_t b) { return a > b ? a : b; }
template <int CTRL>
__device__ __forceinline__ u64_t dpp_u64(u64_t k) {
    const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)k, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(k >> 32), CTRL, 0xF, 0xF, true);
    return ((u64_t)hi << 32) | lo;
}
// acc(2 rows) += w.x * h(2 rows) / w.y * h: v_pk_fma_f32 with the scalar picked by op_sel, so a weight PAIR
// occupies one register pair (the compiler's own splat {w, w} would double the resident weights)
__device__ __forceinline__ void pkfma_lo(f32x2& acc, f32x2 wpair, f32x2 h) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(wpair), "v"(h));
}
__device__ __forceinline__ void pkfma_hi(f32x2& acc, f32x2 wpair, f32x2 h) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(wpair), "v"(h));
}
// acc[4 values][2 row pairs] += w4 (4 values: gates or columns) x h4 (4 rows)
__device__ __forceinline__ void fma_4x4(f32x2 (&acc)[4][2], f32x2 w01, f32x2 w23, float4 hv) {
    const f32x2 h01 = {hv.x, hv.y}, h23 = {hv.z, hv.w};
    pkfma_lo(acc[0][0], w01, h01); pkfma_lo(acc[0][1], w01, h23);
    pkfma_hi(acc[1][0], w01, h01); pkfma_hi(acc[1][1], w01, h23);
    pkfma_lo(acc[2][0], w23, h01); pkfma_lo(acc[2][1], w23, h23);
    pkfma_hi(acc[3][0], w23, h01); pkfma_hi(acc[3][1], w23, h23);
}

