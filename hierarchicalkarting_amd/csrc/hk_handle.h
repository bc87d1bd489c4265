// hk_handle.h — the handle behind hk_handle (include/hk.h) and what both host units of the C ABI do with it: hk_api.hip (the environment: settling,
// the round scheduler, the actors, the rollout recorder, the getters and setters, RCCL, the profiler) and hk_train.hip (the trainers and the snapshot
// pools).  What a trainer may touch of the handle is what this header shows; settling and the scheduler's helpers stay private to hk_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/hk.h"
#include "hk_env_host.h"
#include "hk_policy.h"

#pragma GCC visibility push(hidden)      // nothing below belongs to the C ABI: what crosses the two units stays inside libhk.so

struct hk_context;
namespace hk {
extern thread_local std::string g_last_error;      // hk_last_error(NULL): one object for both units, defined in hk_api.hip
int settle_all(hk_context* h);                     // hk_api.hip: settle(h, SETTLE_ALL) out of line, what HK_NEED_ENV is in hk_train.hip
struct TrainState;                                 // a handle's trainers and snapshot pools (hk_train.hip)
TrainState* train_create();                        // ... empty (nullptr: out of memory)
void train_destroy(hk_context* h);                 // ... every device allocation of theirs freed, then the state itself
// the state of the episode in progress, per [E][A]: what the rows after the last DONE have summed.  whole: the episode's first row lies
// inside the chain of rollouts the carry has been handed along (0: it began before the chain; its end is a partial episode)
struct EpisodeCarry {
    float *ret, *gret;
    int *len, *whole;
};
}  // namespace hk

// HIP-event timing of the kernels on the handle's own stream, without a host sync per launch: every profiled launch is
// bracketed by an event pair taken from a pool; hk_prof_read synchronises once and folds the elapsed times.
struct Prof {
    bool on = false;
    std::vector<hipEvent_t> pool;                                         // free events
    struct Span { hipEvent_t first, second; bool owns_first; };           // owns_first false: `first` is the `second` of the span before
    std::vector<Span> rec[HK_PROF_STAGES];                                // recorded, not yet folded
    double ms[HK_PROF_STAGES] = {};
    int64_t n[HK_PROF_STAGES] = {};
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr;   // (timing stays on; no system-scope fence per record)
        return e;
    }
    // bracket helpers: begin() records the first event of a pair on `st`, end() the second
    hipEvent_t begin(hipStream_t st)
    {
        if (!on) return nullptr;
        hipEvent_t e = get();
        if (e && hipEventRecord(e, st) != hipSuccess) { pool.push_back(e); return nullptr; }
        return e;
    }
    void end(int stage, hipEvent_t e0, hipStream_t st)
    {
        if (!e0) return;
        hipEvent_t e1 = get();
        if (!e1 || hipEventRecord(e1, st) != hipSuccess) { pool.push_back(e0); if (e1) pool.push_back(e1); return; }
        rec[stage].push_back(Span{e0, e1, true});
    }
    // back-to-back launches on one stream share their boundary event: chain() closes the span that began at `prev` and returns the
    // event it recorded as the start of the next one (an event between two kernels costs ~5 us of the GPU's time: a round of
    // {tick kernel, solver kernel} carries two of them this way, not four).  `first`: prev came from begin().
    hipEvent_t chain(int stage, hipEvent_t prev, bool first, hipStream_t st)
    {
        if (!prev) return nullptr;
        hipEvent_t e1 = get();
        if (!e1 || hipEventRecord(e1, st) != hipSuccess) { if (first) pool.push_back(prev); if (e1) pool.push_back(e1); return nullptr; }
        rec[stage].push_back(Span{prev, e1, first});
        return e1;
    }
    void fold()
    {
        for (int s = 0; s < HK_PROF_STAGES; s++) {
            for (auto& pr : rec[s]) {
                float t = 0;
                if (hipEventElapsedTime(&t, pr.first, pr.second) == hipSuccess) { ms[s] += t; n[s]++; }
                if (pr.owns_first) pool.push_back(pr.first);
                pool.push_back(pr.second);
            }
            rec[s].clear();
        }
    }
};

// Scheduling switches: read from the environment ONCE, in hk_create, into the handle (listed in include/hk.h).  None of them changes a result bit; they
// exist for the same-box A/B measurements under profiles/ and for the parity tests that run every schedule against the oracle.  Round 6 retired the ones whose
// A/B is settled (HK_PARK, HK_NO_EAGER, HK_TAIL_WORST_CASE, HK_KEEP_LAST_SOLVE, HK_RUN_CAP_SHORT / _SPREAD, HK_SPLIT_WAYS, HK_SPLIT_MIN_TICKS, HK_LAZY_MIN_TICKS,
// HK_REGROUP_ROUNDS, HK_LQN_SPARSE_BLOCKS, HK_NO_SPLIT, HK_NO_FISSION_SHAPED / _MCTS / _CHUNKS, HK_DEBUG_NO_CHECK, HK_STAMPS_DUMP, HK_LAZY_JOIN, HK_DEBUG_MAX_ROUNDS) with
// their code paths; the numbers they were settled with are in profiles/README.md.  hk_schedule_info() reports what a call ran.
constexpr int LAZY_MIN_TICKS = 64;        // calls at least this long issue the rounds a spread field needs and finish the laggards after a look at the device
// Every call of a plain handle of >= 8 192 envs is split, and a short folded call leaves its parts open for the next one (split_join): hk_step(1) 57.5 us
// on one stream, 72.6 us on two streams joined at the end of every call, 45.7 us joined lazily; hk_step(2) 98.3 / 107.9 / 81.0 us (round 6)
constexpr int SPLIT_WAYS = 2;             // parts of a split batch (three / four parts on as many streams: 1 504 / 1 107 M against 1 532, round 4; three with round 6's in-wave solves: 1 410 against 2 270)
constexpr int LQN_SPARSE_BLOCKS = 1024;   // workgroups per queue of a solver launch once the field has spread
struct Tuning {
    bool fission = true;         // HK_FISSION=0: every handle on the fused tick kernel (phase B1 inside the tick loop) instead of tick kernel + env_b1_kernel per solve cadence
    int split = -1;              // HK_SPLIT=0: one stream always; unset (or 1): every call of a plain handle of >= 8 192 envs runs the batch as two halves on two streams
    int inwave = -1;             // HK_INWAVE=0: multi-player games always go through the queues and a solver launch (the schedule before round 6); 1: env_b1_kernel solves them in-wave in every round (tests); unset: in-wave while the games-per-launch meter says the field has spread
    bool lqn_spread = true;      // HK_LQN=pair: the solver launch of a spread field stays on the pair / matrix-core kernel (the schedule before round 6)
    bool lazy = true;            // HK_FIXED_ROUNDS=1: every call issues the worst-case round count up front (no look at the device)
    bool optimistic = true;      // HK_NO_OPTIMISTIC=1: fixed-round calls always issue the worst-case round count (the schedule before round 5)
    int optimistic_skew = 0;     // HK_OPTIMISTIC_SKEW=k (tests): the believed episode step is off by k, so the exact plans are wrong and the recovery path runs
    bool mcts_pause = true;      // HK_MCTS_NO_PAUSE=1: long calls of planner handles keep the deadline schedule
    bool mcts_overlap = true;    // HK_MCTS_NO_OVERLAP=1: long calls of planner handles launch a replan's searches when its stretch of rounds has ended, on the handle's stream (the schedule before round 5)
    int mcts_side_waves = -1;    // HK_MCTS_SIDE_WAVES=4 / 8 / 0: waves per workgroup of a search launch that runs beside tick launches (unset: 4 where a tick block fits beside one, else 8)
    void read()
    {
        auto flag = [](const char* n) { return std::getenv(n) != nullptr; };
        auto num = [](const char* n, int dflt, int lo, int hi) { const char* e = std::getenv(n); const int v = e ? std::atoi(e) : dflt; return v >= lo && v <= hi ? v : dflt; };
        fission = num("HK_FISSION", 1, 0, 1) != 0;
        split = num("HK_SPLIT", -1, 0, 1);
        inwave = num("HK_INWAVE", -1, 0, 1);
        { const char* e = std::getenv("HK_LQN"); lqn_spread = !(e && std::strcmp(e, "pair") == 0); }
        lazy = !flag("HK_FIXED_ROUNDS");
        optimistic = !flag("HK_NO_OPTIMISTIC"); optimistic_skew = num("HK_OPTIMISTIC_SKEW", 0, 0, 3);
        mcts_pause = !flag("HK_MCTS_NO_PAUSE"); mcts_overlap = !flag("HK_MCTS_NO_OVERLAP");
        { const char* e = std::getenv("HK_MCTS_SIDE_WAVES"); mcts_side_waves = e ? (std::atoi(e) == 4 ? 4 : (std::atoi(e) == 0 ? 0 : 8)) : -1; }
    }
};

struct hk_context {
    int device = 0;
    Tuning tune;
    hipStream_t stream = nullptr;
    hipStream_t qstream[hk::SPLIT_WAYS_MAX - 1] = {};   // the other parts of a split batch run here (issue_rounds)
    bool env_ready = false;
    hk_config cfg{};
    std::vector<hk_section> sections;
    std::vector<hk_wall_seg> walls;
    hk::EnvDevice dev{};           // device-side tables + state
    int* d_status = nullptr;       // LQ singular flag etc.
    std::string err;
    Prof prof;
    // scratch for the host-pointer LQ entry point
    void* lq_scratch = nullptr;
    size_t lq_scratch_bytes = 0;
    // RL policies (hk_policy.h)
    hk::PolicyDevice policy[HK_MAX_POLICIES];
    int n_policies = 0;
    int decision_period = 1;
    long long academy_step = 0;    // ticks stepped since hk_create (Academy.StepCount)
    // lazy completion of hk_step (handles without planner / attached actors): the call issues the rounds a field without
    // multi-player games needs and a guard kernel that reports what is left; the NEXT entry point that touches the state
    // finishes the stragglers (finish_ticks)
    // The optimistic round plan (step_ticks): lock_tick = the episode step every env is believed to stand on (-1: not known) — 0 after a reset of every env,
    // + n per hk_step(n), unknown after anything else that moves episode steps.  A fixed-round call of a plain handle then issues exactly the launches a field
    // in lock-step needs (a tick launch per stretch between solve ticks, a B1 + solver launch per solve tick inside the call) instead of the worst case, and
    // the completion guard VERIFIES it: opt_pending = such a call has been issued and its guard not looked at yet.  The next entry point other than hk_step
    // looks (verify_optimistic): an env the plan missed kept its ticks, the belief is dropped and the laggards are finished like those of a long call.
    long long lock_tick = -1;
    bool opt_pending = false;
    bool exact_plan = false;                 // the current fixed-round call follows the exact plan of a field in lock-step: its last round is the tick launches alone
    int exact_idx = 0, exact_total = 0;      // round counter of the current exact plan (issue_rounds is called in pieces)
    // what else issue_rounds carries from piece to piece of a call (apply_plan / step_ticks set them; finish_ticks and the end of step_rounds clear them)
    bool fold_split = false;                 // a folded call on the two-stream schedule: each part's last tick launch is its completion guard
    int arm_ticks = 0;                       // > 0: a folded call; each part's next tick launch — its first of the call — adds these ticks to every env's count
    int guard_rounds_left = 0;               // > 0: a folded call on one stream; the tick launch that brings it to 0 is the call's last, its guard
    bool last_solve_skippable = false;       // ... of a plain handle: no env can park in that last round, so its solver launch has nothing to solve
    long long mcts_async_deadline = -1;      // short calls of planner handles: the believed episode step at which the search launch running on mcts_stream is first used (-1: none in flight)
    bool step_pending = false;
    bool split = false;            // the current call runs the batch as two halves on two streams (issue_rounds)
    hk::RoundPart parts[hk::SPLIT_WAYS_MAX];    // the parts of the batch, across calls: each keeps its own round and B1-launch counters
    hipEvent_t ev_fork = nullptr, ev_join[hk::SPLIT_WAYS_MAX - 1] = {};
    hipStream_t mcts_stream = nullptr;                  // the search launch of a replan runs here, beside the tick launches up to the plans' deadline (step_ticks, pause mode)
    hipEvent_t ev_mcts_go = nullptr, ev_mcts_done = nullptr;
    int* done_host = nullptr;      // pinned: [0] max ticks left over the envs, [1] an env waits for a queued game
    // the games-per-launch meter (hk_env_device.h GAME_METER): env_b1_kernel keeps, per part of the batch, a decaying maximum of the multi-player games its
    // launches assembled.  A copy travels to pinned memory with every look at the device (lazy completion, the stretches of a planner handle's long call) and,
    // WITHOUT a sync, after a short call — a heuristic may be a call late.  Few games per launch: the B1 waves solve their own (in-wave); many (the Complex
    // track's traffic, envs that reset and bring packs back): queues + the pair solver's launch, 32 games a wave.
    unsigned long long* meter_host = nullptr;     // pinned [4 * GAME_METER_PARTS]
    hipStream_t meter_stream = nullptr;
    int meter_ticks = 0;           // ticks issued since the last copy of a short call
    // Long lazily completed calls (hk_step of thousands of ticks): the host issues far ahead of the GPU and would hold the schedule it chose on entry through
    // whatever the field turns into (second episodes: the resets bring every pack back at once).  A call of >= THROTTLE_MIN_TICKS (64) ticks therefore
    // stays about 8 rounds ahead at most — a marker event every THROTTLE_EVERY (4) rounds, a wait for the marker two back — and looks at the meter at
    // every marker.  The GPU never drains.
    bool throttle = false;
    hipEvent_t ev_thr[4] = {};
    bool thr_valid[4] = {};
    bool split_open = false;       // the parts of the last split call have not been joined into the handle's stream yet (short folded calls: split_join)
    bool meter_was_split = false;  // the call before ran as SPLIT_WAYS parts (their words are the current ones)
    bool meter_looked = false;     // meter_look has run (its band needs a previous answer)
    bool meter_sparse = true;      // what the last copy said (until one arrives: sparse once the field has had BULK_TICKS to spread — launch_b1's rule)
    bool meter_dense = false;      // ... so many games per launch that a solver launch wants the pair solver's 32 games a wave
    int meter_games = 0;           // ... the decaying maximum itself (sizes the spread solver's grid)
    std::string sched;             // hk_schedule_info: the schedule of the last hk_step (written by step_ticks)
    void* pol_scratch = nullptr;   // hk_policy_forward staging
    size_t pol_scratch_bytes = 0;
    // the rollout recorder (hk_rollout_begin ... hk_rollout_close; hk_rollout.h): one allocation behind every HK_RO_* field, then ep_prev[E], bad[1]
    struct Rollout {
        bool open = false;
        int R = 0;                     // rows of the current / last rollout (0: none yet)
        int gen = 0;                   // hk_rollout_begin count (a PPO trainer's advantages belong to one rollout)
        int npol = 0;                  // actors attached when it began (the ones it has rows of)
        int started = 0, rows = 0;     // decisions taken / intervals completed since begin
        int obs_dim = 0, nbm = 0, smax = 1;
        int mem_max = 0;               // the largest 2m of the recurrent actors (0: none; MEMORY / NEXT_MEMORY have no elements)
        uint32_t driven = 0;           // agent slots an actor drives
        void* buf = nullptr;
        size_t bytes = 0;
        size_t off[HK_RO_FIELDS + 2] = {};    // byte offsets; [HK_RO_FIELDS] ep_prev, [HK_RO_FIELDS + 1] bad
        template <typename T> T* at(int f) const { return (T*)((char*)buf + off[f]); }
        // row t of a [R][E][A][k] field
        template <typename T> T* row(int f, int t, size_t ea, int k = 1) const { return at<T>(f) + (size_t)t * ea * k; }
    } ro;
    struct Ppo;                    // a trainer: PPO, POCA, recurrent (hk_train.hip)
    struct Pool;                   // a snapshot pool (hk_train.hip)
    hk::TrainState* train = nullptr;      // the trainers and the pools: hk_create makes it, for the environment-less handle as well
    // the episode statistics of self-play (hk_rollout_episode_stats; hk_selfplay.h); nothing is allocated before the first call
    struct Episodes {
        void* buf = nullptr;           // one allocation: the two carries (ret, gret, len, whole: [E][A] each), the lanes' records [E A], the result [1]
        hk::EpisodeCarry carry[2] = {};
        int in = 0;                    // carry[in] is the current rollout's carry-in, carry[in ^ 1] what the statistics write
        hk_episode_stats* part = nullptr;
        hk_episode_stats* out = nullptr;
        bool moved = true;             // an hk_step / hk_reset / hk_set_*_state / hk_policy_attach ran since the last hk_rollout_close
        int stats_gen[HK_MAX_POLICIES] = {};      // the rollout (Rollout::gen) whose statistics were last computed for the policy
        bool carry_ok[HK_MAX_POLICIES] = {};      // the open / last rollout began with a carry-in adopted for the policy
    } ep;
    // RCCL communicator for hk_gather_results (librccl.so loaded lazily)
    void* comm = nullptr;
    int comm_world = 0, comm_rank = 0;
    void* gather_buf = nullptr;
    size_t gather_bytes = 0;
    void* gather_cnt = nullptr;    // per-rank byte counts of the gather (ranks may hold different env counts)
    size_t gather_cnt_bytes = 0;
};

inline int fail(hk_context* h, int code, const std::string& msg)
{
    hk::g_last_error = msg;
    if (h) h->err = msg;
    return code;
}

#define HK_HIP(h, call)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail((h), HK_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The hk:: launch functions report through h->err only: the thread-local copy (hk_last_error(NULL)) follows here.  Functions that
// went through fail() have set both and are returned from with a plain `if (int rc = ...) return rc;`.
inline int hand_off(hk_context* h, int rc)
{
    if (rc) hk::g_last_error = h->err;
    return rc;
}
#define HK_TRY(h, call) do { if (int rc_ = hand_off((h), (call))) return rc_; } while (0)

// p freed (when it holds anything) and cleared
template <typename T> hipError_t dev_free(T*& p) { T* old = p; p = nullptr; return old ? hipFree(old) : hipSuccess; }

// a device buffer that only grows: below `need` units it is freed and allocated anew at `bytes` (nothing is kept); a failure leaves *p nullptr, *have 0
template <typename T, typename N>
int dev_grow(hk_context* h, T** p, N* have, N need, size_t bytes)
{
    if (need <= *have) return HK_OK;
    *have = 0;
    HK_HIP(h, dev_free(*p));
    HK_HIP(h, hipMalloc((void**)p, bytes));
    *have = need;
    return HK_OK;
}

inline unsigned nblk(size_t n, int b = 256) { return (unsigned)((n + b - 1) / b); }
inline size_t n_karts(const hk_context* h) { return (size_t)h->cfg.num_envs * h->cfg.num_agents; }

// what changes or reads state that an open rollout owns
inline int ppo_refuse_open(hk_handle h, const char* fn)
{
    return h->ro.open ? fail(h, HK_ERR_INVALID, std::string(fn) + ": refused while a rollout is open (hk_rollout_close first)") : HK_OK;
}

#pragma GCC visibility pop
