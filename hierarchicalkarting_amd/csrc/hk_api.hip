// hk_api.hip — C ABI of libhk.so (include/hk.h) on top of the gfx950 kernels.  No CPU fallback anywhere:
// without a HIP device every compute entry point returns HK_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <utility>
#include <algorithm>
#include <new>
#include "../../include/hk.h"
#include "hk_lq_core.h"
#include "hk_env_kernels.h"
#include "hk_policy.h"
#include "hk_rollout.h"
#include "hk_ppo.h"
#include "hk_ppo_lstm.h"
#include "hk_ppo_lstm_critic.h"
#include "hk_poca.h"
#include "hk_selfplay.h"
#include <dlfcn.h>

namespace hk {
// hk_lq_batch.hip
int lq_batch_launch(int batch, int N, const double* dA, const double* dB, const double* dQ, const double* dq, const double* dR,
                    const double* dx0, int horizon, double* du0, int* d_status, hipStream_t st);
}

namespace {

thread_local std::string g_last_error;

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

}  // namespace

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
    // PPO trainers (hk_ppo_*; hk_ppo.h): a master copy of the actor + critic parameters, Adam moments, the rollout's per-row values, and a
    // workspace sized by the largest minibatch seen
    struct Ppo {
        int policy = -1;
        hk::PpoNet actor, critic;
        hk_ppo_config cfg{};
        float* param = nullptr;        // [4][P]: PARAMS, GRAD, ADAM_M, ADAM_V
        size_t P = 0;
        int adam_steps = 0, epochs_done = 0;
        int adv_gen = -1, n = 0;       // the rollout hk_ppo_advantages ran on; its rows
        bool perm_valid = false;       // an hk_ppo_update has written PERM for the current rows
        float* rowbuf = nullptr;       // V_OLD, ADV, RET [n], V_BOOT [E S], PERM (int) [n]
        size_t rowbuf_n = 0;
        void* ws = nullptr;            // minibatch workspace of cap rows (PpoWs, ppo_ws_layout); last_m: the rows of the last minibatch
        int cap = 0, last_m = 0;
        int prec = HK_PPO_PREC_F32;    // hk_ppo_set_precision
        uint16_t* shadow = nullptr;    // HK_PPO_PREC_BF16: PARAMS rounded to bf16, the critic shadow_pad elements on (ppo_shadow_kernel)
        size_t shadow_pad = 0;
        // the running normaliser (hk_ppo_normalizer_*; nothing before init / set): norm_steps 0 = no state
        int64_t norm_steps = 0;        // N
        double* norm = nullptr;        // m [in_dim], M2 [in_dim], then the combined sums [2 in_dim + stack] of an update
        double* norm_part = nullptr;   // an update's per-workgroup partials [norm_part_wg][2 in_dim + stack]
        int norm_part_wg = 0;
        bool adv_stale = false;        // the policy's statistics changed after hk_ppo_advantages: V_OLD is the critic on other inputs
        double* clip = nullptr;        // hk.h "LONG RUNS" (nothing before the first clip-aware step): the HK_PPO_CLIP words [8], then the norm's partials [clip_parts]
        int clip_parts = 0;
        // a POCA trainer (hk.h "POCA"; hk_ppo_create_poca; nothing of this is touched for a PPO trainer): `critic` stays empty, the attention
        // critic's layout is pnet, its rows (B_OLD, TEAM_REWARD [n]) and its minibatch workspace of pcap groups are allocations of their own
        bool poca = false;
        hk::PocaNet pnet;
        float* prow = nullptr;
        size_t prow_n = 0;
        void* pws = nullptr;
        int pcap = 0, last_mg = 0;
        bool lb_from_update = false;   // hk_poca_stats: the last L_b came from an update's accumulator
        // a recurrent trainer (hk.h "PPO trainer" RECURRENT; hk_ppo_create_recurrent; nothing of this is touched for the other kinds): seq_len > 0,
        // the cell and the m-wide heads at lnet's offsets of the actor part (actor.oWmu .. are lnet's), a workspace of its own for rcap rows
        int seq_len = 0, n_seq = 0;
        hk::PpoLstmNet lnet;
        void* rws = nullptr;
        int rcap = 0, last_ms = 0;
        // ... with a recurrent critic (RECURRENT CRITIC; hk_ppo_create_recurrent_critic; nothing of this is touched for the other kinds): critic_m > 0,
        // the critic's cell and value head at cnet's offsets (critic.oWmu / obmu are cnet's W_v / b_v), a minibatch workspace of its own for ccap
        // rows, the memories cmem = MEM_IN | MEM_OUT | the value pass's carry, [E S][2 m_v] each, CRITIC_MEMORY [cmem_k][E S][2 m_v], and the
        // value pass's Zx and summed bias for vcap rows
        int critic_m = 0, value_chunk = 0;
        hk::PpoLstmCriticNet cnet;
        void* cws = nullptr;
        int ccap = 0;
        float* cmem = nullptr;
        float* cmemk = nullptr;
        size_t cmemk_n = 0;
        int cmem_k = 0, cmem_gen = -1;          // windows of the last value pass; the rollout generation MEM_IN belongs to
        float* vws = nullptr;
        size_t vcap = 0;
    } ppo[HK_MAX_POLICIES];
    int n_ppo = 0;
    // self-play (hk.h "SELF-PLAY"; hk_selfplay.h); nothing is allocated before the first hk_policy_pool_create / hk_rollout_episode_stats
    struct Pool {
        int in_dim = 0, stack = 0, hidden = 0, n_layers = 0, n_branch = 0, normalize = 0;    // the SHAPE
        hk::PpoNet net;                // the flat actor layout (base 0); a slot is net.count floats, then mean, std [in_dim] when normalize
        int m = 0;                     // > 0: a recurrent pool (hk_policy_pool_create_recurrent) of memory_size 2m; net is then the trunk alone
        hk::PpoLstmNet lnet;           // (it ends at lnet.oWih) and lnet the cell and the m-wide heads behind it; the actor is lnet.end floats
        size_t actor = 0;              // floats of the actor part of a slot: net.count, or lnet.end for a recurrent pool
        int slots = 0;
        size_t count = 0;              // floats per slot
        float* buf = nullptr;          // [slots][count]
        uint64_t filled = 0;           // bit s: slot s has been written
    } pool[HK_MAX_POOLS];
    int n_pools = 0;
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

static int finish_ticks(hk_context* h);      // lazy completion of the last hk_step (defined with step_ticks)
static int meter_copy(hk_context* h, bool in_order);      // the games-per-launch meter on its way to pinned memory (defined with step_ticks)
static int throttle_mark(hk_context* h, int r);           // long lazy calls: stay a bounded number of rounds ahead of the GPU, look at the meter (defined with step_ticks)
static int verify_optimistic(hk_context* h); // the completion guard of optimistic fixed-round calls, looked at; laggards finished (defined with step_ticks)
static void ppo_release(hk_context::Ppo& t); // every device allocation of a trainer freed, the slot empty again (defined with the PPO trainer)
// a search launch that runs on the side stream beside the chunks of a planner + actor handle (step_ticks): the handle's stream waits for it — before another
// search launch (they share the tree arena), before the chunk that uses its plans, before anything reads the planner state
// Two halves on two streams, JOINED LAZILY (round 6).  A short folded call used to end with its parts' streams joined into the handle's stream — and the next
// call forked them again: a host that steps tick by tick (the reference's FixedUpdate) paid an event pair each way per call and, worse, a GPU-side barrier
// between the calls, so the halves could never drift apart the way they do inside a long call (one half's B1 tail behind the other half's ticks).  Now a
// folded split call leaves its parts open; the next such call just continues on both streams.  Everything else that touches the state — every entry point
// but hk_step, an unsplit or lazily completed call, a regroup — joins first.  (The completion guard's flag is a host word, the meter's copy orders nothing.)
static inline int split_join(hk_context* h)
{
    if (!h->split_open) return 0;
    h->split_open = false;
    for (int k = 0; k < hk::SPLIT_WAYS_MAX - 1; k++) {
        if (!h->qstream[k] || !h->ev_join[k]) continue;
        if (hipEventRecord(h->ev_join[k], h->qstream[k]) != hipSuccess) return -1;
        if (hipStreamWaitEvent(h->stream, h->ev_join[k], 0) != hipSuccess) return -1;
    }
    return 0;
}
static inline int mcts_join_async(hk_context* h)
{
    if (h->mcts_async_deadline < 0) return 0;
    h->mcts_async_deadline = -1;
    return hipStreamWaitEvent(h->stream, h->ev_mcts_done, 0) == hipSuccess ? 0 : -1;
}

namespace {

int fail(hk_context* h, int code, const std::string& msg)
{
    g_last_error = msg;
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
    if (rc) g_last_error = h->err;
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

// Settling the handle before an entry point touches its state, written once: what the calls before left open is brought to the handle's
// stream, in this order.  `what` names the steps; each SETTLE_* constant below is one present use (DESIGN.md §2 "Settling the handle" has the table and says
// which rows are inherited rather than judged).  The mask is a constant at every call site, so each use folds to its own steps.
enum : unsigned {
    SETTLE_ENV = 1,          // the handle must have an environment
    SETTLE_SPLIT = 2,        // join the open parts of a split call (split_join)
    SETTLE_LAZY = 4,         // finish the laggards of a lazily completed call (finish_ticks)
    SETTLE_OPT = 8,          // look at the guard of optimistic fixed-round calls (verify_optimistic)
    SETTLE_MCTS = 16,        // join the planner's side stream (mcts_join_async)
    SETTLE_ALL = SETTLE_ENV | SETTLE_SPLIT | SETTLE_LAZY | SETTLE_OPT | SETTLE_MCTS,      // every entry point that reads or writes the state
    SETTLE_STEP = SETTLE_ENV | SETTLE_LAZY,                   // hk_step: the calls of a host that steps tick by tick follow each other without a look at the device
    SETTLE_SYNC = SETTLE_SPLIT | SETTLE_LAZY | SETTLE_OPT,    // hk_synchronize
    SETTLE_PROF = SETTLE_SPLIT | SETTLE_LAZY,                 // hk_prof_reset, hk_prof_read
    SETTLE_STREAM = SETTLE_SPLIT,                             // hk_stream, which asks only while parts are open
};
__attribute__((always_inline)) inline int settle(hk_context* h, unsigned what)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "NULL handle");
    if ((what & SETTLE_ENV) && !h->env_ready) return fail(h, HK_ERR_INVALID, "handle has no environment");
    HK_HIP(h, hipSetDevice(h->device));
    if ((what & SETTLE_SPLIT) && split_join(h)) return fail(h, HK_ERR_HIP, "hipStreamWaitEvent (the parts of a split call)");
    if ((what & SETTLE_LAZY) && h->step_pending) { int rc = finish_ticks(h); if (rc) return rc; }
    if ((what & SETTLE_OPT) && h->opt_pending) { int rc = verify_optimistic(h); if (rc) return rc; }
    if ((what & SETTLE_MCTS) && mcts_join_async(h)) return fail(h, HK_ERR_HIP, "hipStreamWaitEvent (planner side stream)");
    return HK_OK;
}
#define HK_NEED_ENV(h) do { if (int rc_ = settle((h), SETTLE_ALL)) return rc_; } while (0)

int device_count()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ensure_ctx_basics(hk_context* h)
{
    HK_HIP(h, hipSetDevice(h->device));
    if (!h->stream) HK_HIP(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    if (!h->d_status) {
        HK_HIP(h, hipMalloc(&h->d_status, sizeof(int) * 4));
        HK_HIP(h, hipMemsetAsync(h->d_status, 0, sizeof(int) * 4, h->stream));
    }
    return HK_OK;
}

hk_context* g_default_ctx = nullptr;   // used by hk_lq_solve_batch(NULL, ...)

// The five RCCL entry points hk_gather_results needs, resolved from librccl.so at first use (signatures as in rccl.h;
// ncclUniqueId is a 128-byte struct passed by value, ncclChar = 0, ncclSuccess = 0).
struct RcclId { char internal[HK_COMM_ID_BYTES]; };
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(RcclId*) = nullptr;
    int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool load(std::string& err)
    {
        if (lib) return true;
        lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { err = std::string("hk_comm: cannot load librccl.so: ") + dlerror(); return false; }
        GetUniqueId = (int (*)(RcclId*))dlsym(lib, "ncclGetUniqueId");
        CommInitRank = (int (*)(void**, int, RcclId, int))dlsym(lib, "ncclCommInitRank");
        AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(lib, "ncclAllGather");
        CommDestroy = (int (*)(void*))dlsym(lib, "ncclCommDestroy");
        GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
        if (!GetUniqueId || !CommInitRank || !AllGather || !CommDestroy) { err = "hk_comm: librccl.so lacks an expected symbol"; lib = nullptr; return false; }
        return true;
    }
    std::string why(int rc) const { return GetErrorString ? std::string(GetErrorString(rc)) : std::to_string(rc); }
};
RcclApi g_rccl;

}  // namespace

extern "C" {

const char* hk_last_error(hk_handle h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int hk_create(const hk_config* cfg, hk_handle* out)
{
    if (!out) return fail(nullptr, HK_ERR_INVALID, "hk_create: out is NULL");
    *out = nullptr;
    if (device_count() <= 0) return fail(nullptr, HK_ERR_NO_DEVICE, "hk_create: no HIP device (libhk has no CPU fallback)");
    hk_context* h = new (std::nothrow) hk_context();
    if (!h) return fail(nullptr, HK_ERR_INVALID, "hk_create: out of memory");
    if (cfg) {
        if (cfg->abi_version != HK_ABI_VERSION) { delete h; return fail(nullptr, HK_ERR_INVALID, "hk_create: abi_version mismatch"); }
        h->device = cfg->device_id;
    }
    int rc = ensure_ctx_basics(h);
    if (rc) { g_last_error = h->err; delete h; return rc; }
    h->tune.read();
    if (cfg) {
        h->cfg = *cfg;
        h->dev.regroup_rounds = hk::REGROUP_ROUNDS;
        // the tick kernel without phase B1 + env_b1_kernel per solve cadence for every handle of 3 or 4 agents (hk_env_run.h FISSION).  2-agent fields
        // (cadence 1: every tick is a solve tick and both egos hold the 2-player game, HKA:317,709) stay on the fused kernel: round 6 measured the fission
        // schedule for them (bit-equal; three launches per tick, no eager assembly) at 303 M env-steps/s against the fused kernel's 331 M — with a game
        // per ego and tick the round is the pair solver's 131 072 games (98 us) and the GameSoA round trip of the assembly (B1 82 us), which a split does
        // not shrink.  The 8-lane groups run the older loop.
        h->dev.fission = h->tune.fission && cfg->num_agents > 2 && cfg->num_agents <= 4;
        rc = hk::env_create(h->cfg, h->sections, h->walls, h->dev, h->stream, h->err);
        if (rc) { g_last_error = h->err; hk_destroy(h); return rc; }
        h->env_ready = true;
        if (hipHostMalloc((void**)&h->done_host, 4 * sizeof(int), hipHostMallocDefault) != hipSuccess) h->done_host = nullptr;   // (no pinned memory: fixed rounds)
        else {
            h->done_host[0] = 0; h->done_host[1] = 0; h->done_host[2] = 0; h->done_host[3] = 0;
            // word 2: the completion guards' flag, written by the kernels themselves (EnvParams::guard_flag)
            void* dp = nullptr;
            h->dev.P.guard_flag = hipHostGetDevicePointer(&dp, h->done_host + 2, 0) == hipSuccess ? (int*)dp : nullptr;
        }
        if (hipHostMalloc((void**)&h->meter_host, 4 * hk::GAME_METER_PARTS * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) h->meter_host = nullptr;
        else std::memset(h->meter_host, 0, 4 * hk::GAME_METER_PARTS * sizeof(unsigned long long));
        (void)hipStreamCreateWithFlags(&h->meter_stream, hipStreamNonBlocking);          // (here, not inside a call: creating a stream takes milliseconds)
    }
    *out = h;
    return HK_OK;
}

void hk_destroy(hk_handle h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)split_join(h);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->done_host) (void)hipHostFree(h->done_host);
    if (h->meter_stream) { (void)hipStreamSynchronize(h->meter_stream); (void)hipStreamDestroy(h->meter_stream); }
    for (hipEvent_t e : h->ev_thr) if (e) (void)hipEventDestroy(e);
    if (h->meter_host) (void)hipHostFree(h->meter_host);
    hk::env_destroy(h->dev);
    if (h->d_status) (void)hipFree(h->d_status);
    if (h->lq_scratch) (void)hipFree(h->lq_scratch);
    if (h->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(h->comm);
    if (h->gather_buf) (void)hipFree(h->gather_buf);
    if (h->gather_cnt) (void)hipFree(h->gather_cnt);
    if (h->pol_scratch) (void)hipFree(h->pol_scratch);
    if (h->ro.buf) (void)hipFree(h->ro.buf);
    for (int p = 0; p < HK_MAX_POLICIES; p++) hk::policy_free(h->policy[p]);
    for (auto& t : h->ppo) ppo_release(t);
    for (auto& pl : h->pool) if (pl.buf) (void)hipFree(pl.buf);
    if (h->ep.buf) (void)hipFree(h->ep.buf);
    h->prof.fold();
    for (hipEvent_t e : h->prof.pool) (void)hipEventDestroy(e);
    for (hipStream_t q : h->qstream) if (q) { (void)hipStreamSynchronize(q); (void)hipStreamDestroy(q); }
    if (h->mcts_stream) { (void)hipStreamSynchronize(h->mcts_stream); (void)hipStreamDestroy(h->mcts_stream); }
    if (h->ev_mcts_go) (void)hipEventDestroy(h->ev_mcts_go);
    if (h->ev_mcts_done) (void)hipEventDestroy(h->ev_mcts_done);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (hipEvent_t e : h->ev_join) if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h == g_default_ctx) g_default_ctx = nullptr;
    delete h;
}

void* hk_stream(hk_handle h)
{
    if (!h) return nullptr;
    if (h->split_open && settle(h, SETTLE_STREAM)) return nullptr;       // (work the caller puts on the stream must come behind both parts)
    return (void*)h->stream;
}
const char* hk_schedule_info(hk_handle h) { return h ? h->sched.c_str() : ""; }

int hk_synchronize(hk_handle h)
{
    if (int rc = settle(h, SETTLE_SYNC)) return rc;
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

// ------------------------------------------------------------------ LQ batch
int hk_lq_solve_batch_device(hk_handle h, int batch, int N, const double* dA, const double* dB, const double* dQ,
                             const double* dq, const double* dR, const double* dx0, int horizon, double* du0, void* stream)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "hk_lq_solve_batch_device: handle required");
    if (batch < 0 || N < 1 || horizon < 0) return fail(h, HK_ERR_INVALID, "hk_lq_solve_batch: bad batch/N/horizon");
    if (N > hk::LQ_BATCH_MAXP) return fail(h, HK_ERR_UNSUPPORTED, "hk_lq_solve_batch: N > 8 players not built");
    if (batch == 0) return HK_OK;
    HK_HIP(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    hipEvent_t pe0 = h->prof.begin(st);
    const int rc = hk::lq_batch_launch(batch, N, dA, dB, dQ, dq, dR, dx0, horizon, du0, h->d_status, st);
    const hipError_t le = hipGetLastError();
    if (rc != HK_OK || le != hipSuccess) {
        if (pe0) h->prof.pool.push_back(pe0);          // the opening event of the span goes back to the pool
        if (rc == HK_ERR_UNSUPPORTED) return fail(h, HK_ERR_UNSUPPORTED, "hk_lq_solve_batch: N > 8 players not built");
        return fail(h, HK_ERR_HIP, std::string("hk_lq_solve_batch: kernel launch: ") + hipGetErrorString(le));
    }
    h->prof.end(2, pe0, st);
    return HK_OK;
}

int hk_lq_solve_batch(hk_handle h, int batch, int N, const double* A, const double* B, const double* Q, const double* q,
                      const double* R, const double* x0, int horizon, double* u0_out)
{
    if (!h) {
        if (!g_default_ctx) {
            int rc = hk_create(nullptr, &g_default_ctx);
            if (rc) return rc;
        }
        h = g_default_ctx;
    }
    if (batch < 0 || N < 1) return fail(h, HK_ERR_INVALID, "hk_lq_solve_batch: bad batch/N");
    if (N > hk::LQ_BATCH_MAXP) return fail(h, HK_ERR_UNSUPPORTED, "hk_lq_solve_batch: N > 8 players not built");
    if (batch == 0) return HK_OK;
    if (!A || !B || !Q || !q || !R || !x0 || !u0_out) return fail(h, HK_ERR_INVALID, "hk_lq_solve_batch: NULL pointer");
    HK_HIP(h, hipSetDevice(h->device));
    const size_t n = 4 * (size_t)N, b = (size_t)batch;
    const size_t szA = b * N * 16, szB = b * N * 8, szQ = b * N * n * n, szq = b * N * n, szR = b * N * 4, szx = b * n, szu = b * 2;
    const size_t total = (szA + szB + szQ + szq + szR + szx + szu) * sizeof(double);
    if (int rc = dev_grow(h, &h->lq_scratch, &h->lq_scratch_bytes, total, total)) return rc;
    double* d = (double*)h->lq_scratch;
    double *dA = d, *dB = dA + szA, *dQ = dB + szB, *dq = dQ + szQ, *dR = dq + szq, *dx = dR + szR, *du = dx + szx;
    HK_HIP(h, hipMemcpyAsync(dA, A, szA * 8, hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipMemcpyAsync(dB, B, szB * 8, hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipMemcpyAsync(dQ, Q, szQ * 8, hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipMemcpyAsync(dq, q, szq * 8, hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipMemcpyAsync(dR, R, szR * 8, hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipMemcpyAsync(dx, x0, szx * 8, hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipMemsetAsync(h->d_status, 0, sizeof(int), h->stream));
    int rc = hk_lq_solve_batch_device(h, batch, N, dA, dB, dQ, dq, dR, dx, horizon, du, h->stream);
    if (rc) return rc;
    int st = 0;
    HK_HIP(h, hipMemcpyAsync(u0_out, du, szu * 8, hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipMemcpyAsync(&st, h->d_status, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    if (st & 1) return fail(h, HK_ERR_SINGULAR, "hk_lq_solve_batch: zero pivot in the m x m solve");
    return HK_OK;
}

// ------------------------------------------------------------------ environment
int hk_reset(hk_handle h, const int32_t* env_ids, int n, int experiment_num)
{
    HK_NEED_ENV(h);
    if (h->ro.open) return fail(h, HK_ERR_INVALID, "hk_reset: refused while a rollout is open (hk_rollout_close first)");
    h->ep.moved = true;                         // (the episode statistics' carry ends here: hk.h "SELF-PLAY" CARRY)
    HK_TRY(h, hk::env_reset(h->dev, h->cfg, env_ids, n, experiment_num, h->stream, h->err));
    h->lock_tick = env_ids ? -1 : 0;            // every env stands on episode step 0 again / some do: the field is no longer known to be in lock-step
    // the agents were reset: their observation stacks start from zeros again (env_reset left the ids in dev.env_ids)
    for (int p = 0; p < h->n_policies; p++) {
        const int cnt = (env_ids ? n : h->cfg.num_envs) * h->policy[p].q.n_slots;
        if (cnt <= 0) continue;
        hipLaunchKernelGGL(hk::policy_invalidate_kernel, dim3(nblk(cnt)), dim3(256), 0, h->stream, h->policy[p].q,
                           env_ids ? h->dev.env_ids : nullptr, env_ids ? n : h->cfg.num_envs);
        HK_HIP(h, hipGetLastError());
    }
    return HK_OK;
}

int hk_set_actions(hk_handle h, const float* steer, const int32_t* branch)
{
    HK_NEED_ENV(h);
    if (!steer || !branch) return fail(h, HK_ERR_INVALID, "hk_set_actions: NULL pointer");
    const size_t cnt = n_karts(h);
    HK_HIP(h, hipMemcpyAsync(h->dev.act_steer, steer, cnt * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipMemcpyAsync(h->dev.act_branch, branch, cnt * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

// `rounds` rounds of the batch as K parts (hk_env_host.h RoundPart): the whole batch on the handle's stream or, a split call, SPLIT_WAYS parts (lane groups
// [0, E/2) and [E/2, E), each with its own pair of queue sets) on as many streams.  A round of a part is {tick launch (up to run_cap ticks per env), B1
// launch (the fission schedule), solver launch (the queued multi-player games)} back to back.  Two parts: while one half waits for its handful of solves (one
// solve's latency: 35 - 59 us of an otherwise idle GPU per round — a fifth of a 20-tick call) the other half's tick kernel has the whole GPU.  Nothing is
// deferred: a queued game still costs its env one round.  The streams are joined before anything else touches the state (the guard kernel, a regroup, a getter).
static int issue_rounds(hk_handle h, int rounds)
{
    hk::EnvDevice& d = h->dev;
    const int K = h->split && rounds > 0 ? SPLIT_WAYS : 1, E = h->cfg.num_envs;      // (no round: nothing to fork for)
    hk::RoundPart* const P = h->parts;
    if (K > 1) {
        for (int k = 0; k < K - 1; k++) {
            if (!h->qstream[k]) HK_HIP(h, hipStreamCreateWithFlags(&h->qstream[k], hipStreamNonBlocking));
            if (!h->ev_join[k]) HK_HIP(h, hipEventCreateWithFlags(&h->ev_join[k], hipEventDisableTiming));
        }
        if (!h->ev_fork) HK_HIP(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        // The periodic regroup by solve phase, several parts: counted once per piece of a call and run here, before the fork, where the streams are joined;
        // the rounds issued below count toward the next one, so the count restarts at `rounds`.  (One part: counted round by round, below.)
        if ((d.rounds_since_regroup += rounds) >= d.regroup_rounds) {
            if (split_join(h)) return fail(h, HK_ERR_HIP, "hipStreamWaitEvent (the parts of a split call)");
            HK_TRY(h, hk::env_launch_regroup(d, h->cfg, h->stream, h->err));
            d.rounds_since_regroup = rounds;
        }
    }
    // part k: lane groups [cut(k), cut(k + 1)) — whole blocks of the tick kernel (64 lane groups; 128 in its 512-thread form).  Part 0 of an unsplit call
    // is everything, and continues the parity of its queue sets 0 / 1 where the call before — split or not — left it.
    auto cut = [&](int k) { return k == K ? E : (int)(((long long)E * k / K + 127) / 128 * 128); };
    for (int k = 0; k < K; k++) { P[k].stream = k ? h->qstream[k - 1] : h->stream; P[k].index = k; P[k].slot0 = cut(k); P[k].slot1 = cut(k + 1); }
    if (K > 1 && !h->split_open) {          // (open: the call before left its parts on these streams — this one continues them)
        HK_HIP(h, hipEventRecord(h->ev_fork, h->stream));
        for (int k = 1; k < K; k++) HK_HIP(h, hipStreamWaitEvent(P[k].stream, h->ev_fork, 0));
    }
    if (K > 1) h->split_open = true;
    hipEvent_t e[hk::SPLIT_WAYS_MAX];       // one profiler event chain per part
    for (int k = 0; k < K; k++) e[k] = h->prof.begin(P[k].stream);
    const bool b1 = d.fission && d.P.any_lqr != 0;      // the fission schedule: a tick launch parks its envs at their solve tick, env_b1_kernel is next on that stream
    const int cadence = hk::solve_cadence(h->cfg);
    // a folded call arms inside each part's first tick launch of its first piece (no env_arm_kernel in front of the fork)
    const int arm = h->arm_ticks;
    bool first = true;
    int rc = HK_OK;
    // Round 6, from the kernel trace of the driver's 20-tick call (profiles/r06_b_short_call_trace.txt): the HOST is what the GPU waits for at the start of a
    // short call — a launch costs it 6 - 8 us, and with one part's whole round issued before the other's first launch the second stream began 93 us into a
    // 895 us call.  The launches of a round are therefore issued kind by kind: every part's tick launch, then every part's B1 launch, then the solver launches.
    for (int r = 0; r < rounds && rc == HK_OK; r++) {
        if ((rc = throttle_mark(h, r))) break;
        // the periodic regroup, one part: counted per round — it may fall between two rounds of a call
        if (K == 1 && ++d.rounds_since_regroup >= d.regroup_rounds && (rc = hk::env_launch_regroup(d, h->cfg, h->stream, h->err))) break;
        // The completion guard of a folded call (no env_check_kernel behind it; lazy and pause calls have none).  One part: the tick launch that ends the
        // countdown over all the pieces of the call.  A folded split call (one piece): each part's tick launch in the last round.
        const bool guard = K > 1 ? h->fold_split && r == rounds - 1 : h->guard_rounds_left > 0 && --h->guard_rounds_left == 0;
        const bool plan_last = h->exact_plan && ++h->exact_idx == h->exact_total;      // (once per round, not per part)
        for (int k = 0; k < K && rc == HK_OK; k++) {
            if ((rc = hk::env_launch_run(d, h->cfg, P[k], r == 0 ? arm : 0, guard, h->err))) break;
            e[k] = h->prof.chain(0, e[k], first, P[k].stream);
        }
        h->arm_ticks = 0;
        first = false;
        if (rc) break;
        if (plan_last) {            // the exact plan's last round is the tick launches alone: no solve tick is left in the call
            for (int k = 0; k < K; k++) P[k].round += 1;
            continue;
        }
        // in-wave solves (hk_lq_spread.h lqs_inwave) once the field has spread — while it stands close (BULK_TICKS after a reset of every env) nearly every ego
        // holds a game and the queues + the pair solver's 32 games per wave are several times cheaper per game  (HK_INWAVE=1, tests: in every round)
        const bool inwave = b1 && hk::inwave_now(d);
        for (int k = 0; b1 && k < K && rc == HK_OK; k++) {
            if ((rc = hk::env_launch_b1(d, h->cfg, P[k], inwave, h->err))) break;
            P[k].b1_launches += 1; P[k].meter_stale = false;          // (the launch counted into its meter slot and started stale words over)
            e[k] = h->prof.chain(5, e[k], false, P[k].stream);
        }
        // The guard of a fixed-round call of a plain handle on one stream was the call's last tick launch: an env that queued a game there would be parked,
        // i.e. the call incomplete, which the round count rules out.  The skip is verified ON THE DEVICE by that very launch: as the guard it raises status
        // bit 2 for any env it leaves with ticks or a phase (a parked env has phase 1 or 2), and the next getter reports it.  Nothing to solve: a one-tick
        // call is 3 launches, not 4.
        const bool skip = guard && h->last_solve_skippable;
        for (int k = 0; k < K && rc == HK_OK; k++) {
            if ((rc = hk::env_launch_lqn(d, h->cfg, P[k], inwave, skip, h->err))) break;
            if (!inwave) e[k] = h->prof.chain(1, e[k], false, P[k].stream);          // (a skipped launch still is a solver stage to the profiler, an in-wave round has none)
            P[k].round += 1;
            // a round retires at least one solve cadence; counted with part 0 only, at once: the next part's solver launch already sizes its grid by it
            if (k == 0) d.call_ticks_issued = std::min(d.call_ticks_issued + cadence, d.call_ticks);
        }
    }
    if (first) for (int k = 0; k < K; k++) if (e[k]) h->prof.pool.push_back(e[k]);          // no round issued: the opening events go back
    // a folded split call (nothing follows its rounds on the handle's stream: no guard kernel, no report) leaves its parts open for the next one; any other
    // call, and any error, joins
    if (K > 1 && (!h->fold_split || rc) && split_join(h) && !rc) rc = fail(h, HK_ERR_HIP, "hipStreamWaitEvent (the parts of a split call)");
    return hand_off(h, rc);
}

// guard kernel + (lazy mode) its report on the way to pinned host memory
static int issue_check(hk_handle h, bool lazy)
{
    if (lazy) HK_HIP(h, hipMemsetAsync(h->dev.status + 1, 0, 2 * sizeof(int), h->stream));
    HK_TRY(h, hk::env_launch_check(h->dev, h->cfg, lazy, h->stream, h->err));
    if (lazy) HK_HIP(h, hipMemcpyAsync(h->done_host, h->dev.status + 1, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (lazy) return meter_copy(h, true);          // (the caller synchronises before it looks at either)
    return HK_OK;
}

// Lazy completion: wait for the last hk_step's report; while some env still has ticks to run (it met multi-player games, each
// of which costs it a round), issue the rounds the laggard needs and look again.
static int finish_ticks(hk_handle h)
{
    h->last_solve_skippable = false; h->guard_rounds_left = 0; h->exact_plan = false; h->throttle = false;      // (the laggards' rounds are plain rounds)
    bool packed = false;
    for (int guard = 0; guard < 1024 && h->step_pending; guard++) {
        HK_HIP(h, hipStreamSynchronize(h->stream));
        const int maxleft = h->done_host[0], waiting = h->done_host[1];
        if (maxleft <= 0 && !waiting) { h->step_pending = false; break; }
        HK_TRY(h, hk::env_launch_regroup(h->dev, h->cfg, h->stream, h->err));      // the laggards into the first lane groups
        packed = true;
        h->split = false;                // ... which all lie in the first half: the tail runs as one batch on one stream (part 0: its round parity goes on)
        // Rounds for the slowest env if it met no further multi-player game (+ 1), not for the worst case (a round per cadence): the
        // batch ends with a look at the device anyway, and two thirds of the worst-case rounds used to find nothing to do (94 of 141 in
        // the headline's 3 072-tick call, ~18 us each).  An env that does park on every solve tick still gets a third of its ticks per batch.
        const int cap = std::max(h->dev.P.run_cap, hk::solve_cadence(h->cfg));
        if (int rc = issue_rounds(h, (maxleft + cap - 1) / cap + 1)) return rc;
        if (int rc = issue_check(h, true)) return rc;
    }
    if (h->step_pending) { h->step_pending = false; return fail(h, HK_ERR_HIP, "hk_step: an env did not complete its ticks (internal scheduling error)"); }
    // The laggards — the envs that met the most multi-player games, and will meet the next ones — now sit side by side in the first lane groups.  With the
    // games solved in-wave that is the worst order there is (a wave solves its games a pass at a time, and the whole front of the batch is one half of a
    // split call): the next round regroups again, and with every env done that regroup spreads the envs that hold games evenly (hk_regroup_pos.h).
    // Found in the driver's window: B1 launches of 91 us where the same games, never packed, took 73 (profiles/r06_f_spread_regroup.txt).
    // (whatever the schedule is now: the next call decides again, and its regroup packs or spreads accordingly)
    if (packed) h->dev.rounds_since_regroup = h->dev.regroup_rounds;
    return HK_OK;
}

// may the B1 launches of this call solve their games in-wave?  (the fission schedule of a quad handle with LQ agents; per round launch_b1 still keeps
// the queues while the field stands close after a reset of every env)
static bool inwave_allowed(hk_handle h)
{
    if (!h->dev.fission || h->dev.P.any_lqr == 0 || h->tune.inwave == 0) return false;
    return h->tune.inwave == 1 || h->meter_sparse;
}
constexpr int METER_TICKS = 16;
// the meter's copy to pinned memory: on the handle's stream (the caller synchronises: the copy is current) or, after a short call, on a stream of its own
// (the copy orders nothing and must not stand between two launches of the handle's stream; it shows whatever the device has reached)
static int meter_copy(hk_handle h, bool in_order)
{
    if (!h->meter_host || !h->dev.game_stats) return HK_OK;
    hipStream_t st = h->stream;
    if (!in_order) {
        if (!h->meter_stream) return HK_OK;
        st = h->meter_stream;
    }
    HK_HIP(h, hipMemcpyAsync(h->meter_host, h->dev.game_stats + hk::GAME_METER, 4 * hk::GAME_METER_PARTS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    return HK_OK;
}
// what the last copy says (the three regimes and their borders: below)
static void meter_look(hk_handle h)
{
    if (!h->meter_host) return;
    // (the parts the call before ran as: a part that no longer launches keeps its last word for ever — a host that steps tick by tick after a race start on two
    // streams would read the start's counts from the idle part for the rest of the race; a part that launches again after a change of shape starts its words over)
    const int parts = h->meter_was_split ? SPLIT_WAYS : 1;
    unsigned long long worst = 0;
    for (int p = 0; p < parts; p++) worst = std::max(worst, h->meter_host[4 * p + 3]);
    const double envs_per_launch = h->cfg.num_envs / (double)parts;
    // Three regimes, by the games of a launch of `envs_per_launch` envs (same-box A/Bs: profiles/r06_f_spread_regroup.txt — 20-tick windows along the race
    // start with the games solved in-wave and by a solver launch —, r06_b_short_call_trace.txt, r06_c_dense_fields.txt):
    //   up to 1 per 40 envs    in-wave (per half-batch launch of 32 768 envs: 2 - 7 % ahead of a solver launch at 54 .. 722 games, 11 % behind at 2 779; a wave
    //                          that holds games runs one pass while the regroup keeps such envs apart)
    //   up to 1 per 8 envs     queues + lqn_spread_kernel, its grid sized for the count
    //   beyond                 queues + the pair / matrix-core kernel, 32 games a wave (the Complex track under the planner: 101.8 against 57.5 M; second episodes: 1 412 against 772 M)
    // (with a band: a field that hovers at a border would change sides call by call, and every change of sides is a regroup)
    h->meter_sparse = (double)worst <= envs_per_launch / 40.0 || (h->meter_sparse && h->meter_looked && (double)worst <= envs_per_launch / 28.0);
    h->meter_looked = true;
    h->meter_dense = (double)worst > envs_per_launch / 8.0;
    h->meter_games = (int)std::min<unsigned long long>(worst, 1u << 30);
}

// what the meter's last look means for the launches from here on: where the multi-player games are solved, and — the two are coupled — how the regroup
// orders the envs that hold them.  Queues want such envs PACKED (they leave their tick launches together), in-wave solves want them APART (a wave solves
// its games a pass at a time; hk_regroup_pos.h): when the schedule changes sides the order of the last regroup is the wrong one, so the next round regroups.
static void apply_meter(hk_handle h)
{
    h->dev.inwave_ok = inwave_allowed(h);
    h->dev.dense = h->meter_dense || !h->dev.fission;      // (the meter lives in env_b1_kernel: a handle on the fused kernel keeps round 5's solver launch)
    h->dev.lqn_sparse_blocks = std::min(4096, std::max(LQN_SPARSE_BLOCKS, h->meter_games));
    if (h->dev.regroup_mode >= 0 && h->dev.regroup_mode != (hk::inwave_now(h->dev) ? 1 : 0)) h->dev.rounds_since_regroup = h->dev.regroup_rounds;
}
// (round 6, end: a marker every 4 rounds and in every lazily completed call — every 16 rounds and in calls of >= 512 ticks before.  The races of a batch that
// was reset together END together: within ~150 ticks the field goes from a few dozen games per launch to a game for every ego, and a host that looked every
// 16 rounds from up to 48 rounds ahead kept the in-wave schedule through ~60 rounds of that — B1 launches of milliseconds (tools/experiments/schedule_trace.py:
// 110 ms of B1 in the 200-tick call that held the onset, 22.7 ms now; second episodes 1 409 -> 1 626 M, the windows at ticks 20 000 / 40 000 1 342 / 1 336 ->
// 1 565 / 1 544 M; profiles/r06_g_long_run.txt).  The host issues a round in ~25 us, the GPU runs one in ~115: 8 - 12 rounds of queued work never drain —
// the protocol window, the race start and the short calls read the same.  Sending the games of three and more players of such a field to a solver launch of
// their own (four of them sit in ONE quad when an env restarts) was built, parity-green, and lost to this: 1 445 - 1 463 M against 1 544 - 1 565.)
// (a marker every 1 / 2 / 4 / 8 rounds, same box: second episodes 1 656 / 1 674 / 1 632 / 1 489 M, ticks 20 000 .. 26 000 1 589 / 1 586 / 1 575 / 1 493 M, protocol window
// 2 279 / 2 303 / 2 314 / 2 321 M: 4 keeps a millisecond of queued work between a descheduled host thread and an idle GPU)
constexpr int THROTTLE_EVERY = 4, THROTTLE_MIN_TICKS = 64;
static int throttle_mark(hk_handle h, int r)
{
    if (!h->throttle || (r % THROTTLE_EVERY) != THROTTLE_EVERY - 1) return HK_OK;
    const int i = (r / THROTTLE_EVERY) & 3, back = (i + 2) & 3;
    if (h->thr_valid[back]) HK_HIP(h, hipEventSynchronize(h->ev_thr[back]));          // the GPU has passed the marker of 2 x THROTTLE_EVERY rounds ago
    meter_look(h);
    apply_meter(h);
    if (!h->ev_thr[i]) HK_HIP(h, hipEventCreateWithFlags(&h->ev_thr[i], hipEventDisableTiming));
    HK_HIP(h, hipEventRecord(h->ev_thr[i], h->stream));
    h->thr_valid[i] = true;
    return meter_copy(h, false);
}

// Everything one hk_step call of n_ticks runs, decided in one place from the handle as the call finds it (plan_call writes nothing; step_ticks
// applies the plan and issues it):
//   planner            the handle has MCTS agents; lat_min the smaller of its two latencies; a short_call (n_ticks <= defer) shares one search launch
//                      with the calls around it; T0 the episode step the field is believed to stand on before the call (-1: not known); t_req >= 0: a
//                      short call of a planner + actor handle that holds the replan step t_req — its searches go to the side stream
//   pause              long call of a planner handle without actors: stretches of rounds between search launches (step_pause)
//   lazy               the rounds a field without multi-player games needs; the laggards are finished by the next entry point (finish_ticks)
//   fold               the first tick launch arms and the last one is the completion guard (no env_arm_kernel, no env_check_kernel)
//   split              two halves on two streams (issue_rounds); fold_split: each part's last tick launch is its guard; continue_split: a short
//                      folded split call continues the parts the call before left open
//   eager, run_cap     P.eager (the eager assembly, hk_env_run.h) and P.run_cap (ticks an env may run per launch)
//   throttle           stay a bounded number of rounds ahead of the GPU and look at the meter (throttle_mark)
//   rounds             rounds issued up front (pause: 0, the stretches decide); exact_plan: the optimistic plan, exactly `rounds` launches
//   last_solve_skippable, guard_rounds_left    -> the handle, for issue_rounds; rounds_mode: hk_schedule_info's "rounds"
struct CallPlan {
    int n_ticks = 0, lat_min = 0, defer = 0;
    long long T0 = -1, t_req = -1;
    bool planner = false, short_call = false, pause = false, lazy = false, fold = false, split = false, fold_split = false, continue_split = false;
    bool eager = false, throttle = false, exact_plan = false, last_solve_skippable = false;
    int run_cap = hk::RUN_CAP, rounds = 0, guard_rounds_left = 0;
    const char* rounds_mode = "";
};

static CallPlan plan_call(const hk_context* h, int n_ticks)
{
    const hk_config& cfg = h->cfg;
    const bool quad = cfg.num_agents > 2 && cfg.num_agents <= 4, fission = h->dev.fission, any_lqr = h->dev.P.any_lqr != 0;
    CallPlan p;
    p.n_ticks = n_ticks;
    // Planner searches: a launch of the search kernel lasts as long as one search however few it holds, so requests are batched.  A long call launches
    // them every MCTS_FLUSH_ROUNDS rounds and once more before it returns; short calls (a Unity host stepping tick by tick, or the chunks between two RL
    // decisions) share ONE launch until `defer` ticks have been armed since the last one — early enough, because a plan is due > MCTS_MIN_LATENCY ticks
    // after its request.  (hk_get_mcts_state launches what is pending before it reads.)  A request posted on armed tick 1 is searched before armed
    // tick defer + 1 runs, and its plan is due `latency` ticks after the request: defer = the handle's smaller latency - 1, at least MCTS_DEFER_TICKS.
    p.planner = h->dev.mcts.st != nullptr;
    const bool plain = !p.planner && h->n_policies == 0;
    p.lat_min = std::min(cfg.mcts_latency_ticks, cfg.mcts_initial_latency_ticks);
    p.defer = std::max(hk::MCTS_DEFER_TICKS, p.lat_min - 1);
    p.short_call = p.planner && n_ticks <= p.defer;
    p.T0 = h->lock_tick;
    // Round 5: the searches of a replan beside the CHUNKS that follow it (handles with attached actors step in decision chunks; round 4 launched a replan's
    // searches up to `defer` ticks late, on the handle's stream, and every chunk behind them waited ~10 - 100 ms).  If the field is believed to be in lock-step
    // the host knows the chunk that holds the replan step (a multiple of 100): whatever is queued is searched BEFORE that chunk, so that the launch after it
    // holds that chunk's requests only — none older than the chunk — and may therefore run on the side stream until the chunk that reaches request +
    // latency.  A wrong belief costs the overlap only: requests posted at other times are served by the `defer` rule exactly as before, and every
    // search launch first waits for the one in flight (they share the tree arena).
    if (p.short_call && p.T0 >= 0 && h->tune.mcts_overlap && h->n_policies > 0 && (p.T0 / 100 + 1) * 100 <= p.T0 + n_ticks) p.t_req = (p.T0 / 100 + 1) * 100;
    // Long calls of a planner handle without attached actors run in PAUSE mode: an env that requests a search stops at the next tick boundary until the
    // search has run, the host runs a stretch of rounds (every env reaches its replan tick or the end of the call), launches ALL the searches of the stretch
    // in one batch, looks at what is left and repeats.  Without the pause the requests of one replan wave trickle in over many rounds (envs that queue
    // multi-player games advance 4 ticks a round, the others 8) and every partial batch costs a full search latency: 4-agent Complex, 16 384 envs: 11.8 -> see profiles/.
    p.pause = p.planner && !p.short_call && h->n_policies == 0 && h->done_host != nullptr && h->tune.mcts_pause;
    // Rounds.  An env that meets no multi-player game retires RUN_CAP ticks per round; one that does retires at least a solve cadence.  Handles with a
    // planner or attached actors issue the worst-case count up front (they step in short chunks and must not stall on the host).  Everything else — the
    // LQNG races of the headline — issues what a field without multi-player games needs, and the stragglers are finished lazily by the next call that
    // touches the state (finish_ticks): most of the worst-case rounds found nothing to do, and on a 20-tick call they were 5 launches of 8.  (Short calls —
    // a host stepping tick by tick — keep the fixed count too: a handful of rounds, no host sync.)
    p.lazy = plain && h->done_host != nullptr && n_ticks >= LAZY_MIN_TICKS && h->tune.lazy;
    // Arming: a kernel of its own for pause and lazy calls; in the others the first tick launch adds the ticks itself and the last one raises the "did not
    // complete" flag the guard kernel would (a one-tick call: 4 launches instead of 9 with round 2's tail regroup; split calls fold too since round 6)
    p.fold = !p.pause && !p.lazy;
    // the eager assembly (hk_env_run.h) for plain quad handles, and in pause mode too: requests are posted on the same ticks, a round earlier at most
    // (configs[2]: 61.4 -> 63.6 M env-steps/s).  Planner / actor handles outside pause mode keep their deadline arithmetic as it was.
    p.eager = quad && (plain || p.pause);
    // Two halves on two streams (issue_rounds) for every call of a plain handle of >= 8 192 envs: round 4 split the long calls (1 472 vs 1 392 M
    // env-steps/s in round 3's protocol window; headline 1 221 -> 1 292 M, race start 439 -> 458 M), round 6 every call, with the parts joined lazily.
    p.split = plain && p.eager && h->tune.split != 0 && cfg.num_envs >= 8192;
    p.fold_split = p.fold && p.split;
    p.continue_split = p.fold_split && h->tune.lazy && n_ticks < LAZY_MIN_TICKS;
    p.throttle = p.lazy && n_ticks >= THROTTLE_MIN_TICKS && fission && any_lqr;
    // ticks per launch: FISSION — every env parks at every solve tick, so a round retires exactly one cadence; longer launches once the field has spread
    // out (RUN_CAP_SPREAD); short calls of plain LQNG handles one solve cadence per launch — with the eager assembly every env, in a pack or not, retires
    // it, so a 20-tick call is 6 equal rounds and no tail (at 8 ticks per launch: 3 rounds + a regroup + 5 rounds for the laggards)
    const long long since_reset = h->dev.ticks_since_reset + h->dev.call_ticks;        // (the call before counts from here on)
    if (p.pause) p.run_cap = fission ? 4 : hk::RUN_CAP;
    else if (fission && any_lqr) p.run_cap = 4;
    else if (p.lazy && cfg.num_agents > 2 && since_reset >= hk::BULK_TICKS) p.run_cap = hk::RUN_CAP_SPREAD;
    else if (!p.lazy && p.eager) p.run_cap = 4;
    if (p.pause) p.rounds = 0;
    else if (p.lazy) p.rounds = hk::env_rounds_min(n_ticks, p.run_cap);
    else p.rounds = hk::env_rounds_for(cfg, n_ticks, p.run_cap, p.eager);
    // The optimistic plan of a fixed-round call (round 5).  If every env stands on episode step T0, the call's ticks T0 + 1 .. T0 + n hold S solve ticks
    // (multiples of the cadence) and the field needs exactly S rounds of {tick launch up to the solve tick, B1, solver} and one more tick launch: a one-tick
    // call off a solve tick is ONE launch, the driver's 20-tick window 6 + 5 + 5 launches per half instead of 7 + 7 + 7.  The plan is a belief, not a proof
    // (envs finish and reset on their own; a time-out inside the call would add a solve tick): the call's completion guard verifies it, an env the plan
    // missed keeps its ticks (and stays parked at its solve tick: hk_env_run.h `stuck`), and the next entry point that looks at the state drops the belief
    // and finishes it (verify_optimistic).  Nothing is ever wrong, a wrong belief is only slow — so it is used only where it is cheap to check.
    if (!p.lazy && plain && fission && any_lqr && h->tune.optimistic && p.T0 >= 0 && p.T0 + n_ticks < cfg.max_episode_steps) {
        const long long Tb = p.T0 + h->tune.optimistic_skew;
        const int cad = hk::solve_cadence(cfg);
        p.rounds = (int)((Tb + n_ticks) / cad - Tb / cad) + 1;               // the multiples of the cadence in (Tb, Tb + n], + 1
        p.exact_plan = true;
    }
    p.guard_rounds_left = p.fold && !p.split ? p.rounds : 0;         // the tick launch that brings this to 0 is the call's last: it is the guard
    p.last_solve_skippable = p.fold && plain && !p.split;
    p.rounds_mode = p.pause ? "pause (stretches of rounds between search launches)" : p.lazy ? "lazy" : "fixed";
    return p;
}

// hk_schedule_info: what the call just issued ran (bench.py prints it, so a measured number names its schedule)
static void record_schedule(hk_handle h, const CallPlan& p)
{
    char buf[640];
    const char* kern = h->dev.fission ? "fission (tick kernel + env_b1_kernel per solve cadence)" : "fused";
    const char* games = !h->dev.fission || h->dev.P.any_lqr == 0 ? "queues + solver launch"
                        : (h->dev.inwave_ok ? (h->dev.inwave_always ? "in-wave (env_b1_kernel), every round" : "in-wave (env_b1_kernel) once the field has spread, queues + solver launch before")
                                            : (h->dev.lqn_spread ? "queues + lqn_spread_kernel (lqn_round_kernel while the field stands close)" : "queues + lqn_round_kernel"));
    std::snprintf(buf, sizeof(buf),
                  "{\"call_ticks\": %d, \"rounds\": \"%s\", \"rounds_issued\": %d, \"kernel\": \"%s\", \"streams\": %d, \"ticks_per_launch\": %d, "
                  "\"optimistic_plan\": %s, \"armed_in_first_launch\": %s, \"multi_player_games\": \"%s\", \"games_meter\": \"%s\", \"games_meter_value\": %d, \"planner\": %s, \"actors\": %d}",
                  p.n_ticks, p.rounds_mode, p.rounds, kern, p.split ? SPLIT_WAYS : 1, p.run_cap, p.exact_plan ? "true" : "false", p.fold ? "true" : "false",
                  games, h->meter_sparse ? "sparse" : (h->meter_dense ? "dense" : "medium"), h->meter_games, p.planner ? "true" : "false", h->n_policies);
    h->sched = buf;
}

// the plan into the handle (the order matters where noted)
static void apply_plan(hk_handle h, const CallPlan& p)
{
    if (h->lock_tick >= 0) h->lock_tick += p.n_ticks;
    if (p.short_call) h->dev.mcts_ticks += p.n_ticks;
    h->dev.mcts_defer = p.short_call || p.pause;            // (pause: the host launches the searches between the stretches, the rounds do not)
    h->dev.ticks_since_reset += h->dev.call_ticks;      // the previous call's ticks
    h->dev.lqn_spread = h->tune.lqn_spread;
    h->dev.inwave_always = h->tune.inwave == 1;
    h->dev.call_ticks = p.n_ticks; h->dev.call_ticks_issued = 0;
    h->dev.P.mcts_pause = p.pause ? 1 : 0;
    h->dev.P.eager = p.eager ? 1 : 0;
    h->dev.P.run_cap = p.run_cap;
    h->throttle = p.throttle;
    for (bool& v : h->thr_valid) v = false;
    h->split = p.split;
    if (h->split != h->meter_was_split && h->dev.game_stats) {
        // the batch changes shape: the parts that stop launching (or start again after a long time) must not be read with their old words
        // (no launch for it: the parts' next B1 launches start their words over, the host reads only the parts a call ran as — meter_look)
        for (int k = 1; k < hk::SPLIT_WAYS_MAX; k++) h->parts[k].meter_stale = true;
        h->meter_was_split = h->split;
    }
    apply_meter(h);                                     // (after P.eager and the previous call's ticks)
    h->exact_plan = p.exact_plan;
    h->exact_idx = 0; h->exact_total = p.rounds;           // (read only while exact_plan is set)
    h->guard_rounds_left = p.guard_rounds_left;
    h->fold_split = p.fold_split;
    h->last_solve_skippable = p.last_solve_skippable;
}

// A search launch on the side stream, behind everything issued so far on the handle's stream; the handle's stream waits for ev_mcts_done before anything
// uses its plans (mcts_join_async, or step_pause itself)
static int launch_side_search(hk_handle h, int side_waves)
{
    if (!h->mcts_stream) HK_HIP(h, hipStreamCreateWithFlags(&h->mcts_stream, hipStreamNonBlocking));
    if (!h->ev_mcts_go) HK_HIP(h, hipEventCreateWithFlags(&h->ev_mcts_go, hipEventDisableTiming));
    if (!h->ev_mcts_done) HK_HIP(h, hipEventCreateWithFlags(&h->ev_mcts_done, hipEventDisableTiming));
    HK_HIP(h, hipEventRecord(h->ev_mcts_go, h->stream));
    HK_HIP(h, hipStreamWaitEvent(h->mcts_stream, h->ev_mcts_go, 0));
    h->dev.mcts_side_waves = side_waves;
    HK_TRY(h, hk::env_flush_mcts_on(h->dev, h->stream, h->mcts_stream, h->err));
    HK_HIP(h, hipEventRecord(h->ev_mcts_done, h->mcts_stream));
    return HK_OK;
}

// Pause mode: stretches of rounds, each ended by a search launch and a look at what is left (the fission schedule for planner handles too: the same two
// kernels with the planner hooks, round 4)
static int step_pause(hk_handle h, const CallPlan& p)
{
    const int cadence = hk::solve_cadence(h->cfg);
    // Search workgroups beside the ticks: 4 waves (one per SIMD) on EVERY CU when a tick block still fits a CU's LDS beside one — the searches then run
    // a wave to a SIMD (~7 ms instead of ~10.6 at two waves per SIMD on half the CUs); phase B1 reads its tables from global memory and the solver
    // launch takes its <= 256-register form for those rounds (b1_small; hk_env_launch.h).  Otherwise 8 waves on half the CUs (round 5's first form).
    int sw = h->dev.tab_lds ? 4 : 8;
    for (int c = 0; c < h->dev.n_mcls; c++) {
        const auto& K = h->dev.mcls[c];
        if (hk::ga_ops(h->dev).mcts_lds_bytes(K.ntab, h->dev.P.L, K.na, K.lds_tier, 4) + (size_t)h->dev.tab_lds + 1024 > 160 * 1024) sw = 8;
    }
    if (h->tune.mcts_side_waves >= 0) sw = h->tune.mcts_side_waves;
    // Round 5: a replan's searches run BESIDE the ticks that follow it.  The reference's search thread works for T = 0.9 s while FixedUpdate goes on
    // (HKA:172-284) and its plan is used mcts_latency_ticks after the request; an env with an outstanding search now steps on until that tick
    // (hk_env_run.h held_now) instead of stopping at once, so the search launch — as long as ONE search whatever the batch, ~10 ms — can share the GPU
    // with up to 44 ticks of every env.  The host does not know when requests are posted; it guesses from the ticks since the last reset of every env
    // (a field that was reset together replans together, on episode steps that are multiples of 100): the stretch is cut to end 40 ticks after the next
    // such step, the searches are launched on a side stream right after the round that is expected to post the requests, and the handle's stream waits
    // for them only before the rounds that could reach the deadline.  A wrong guess costs the overlap, nothing else: every stretch still ends with a
    // search launch for whatever is queued, and no env passes its deadline unserved (device side).
    const bool overlap = h->tune.mcts_overlap && h->dev.fission && cadence == 4 && p.lat_min >= 24;
    int rc, maxleft = p.n_ticks;
    for (int guard = 0; guard < 4096; guard++) {
        // a stretch: enough rounds for EVERY env to reach its next replan (<= 100 ticks away) or the end of the call, also one that meets a multi-player
        // game on every solve tick (a solve cadence per round).  The rounds in which most envs already wait cost tens of microseconds; a second search
        // launch for the late ones would cost a full search latency
        int reach = std::min(maxleft, 100);
        int r_post = -1, r_free = 0;
        if (overlap) {
            const long long T = (long long)h->dev.ticks_since_reset + (p.n_ticks - maxleft);      // episode step of a field in lock-step
            const int k = 100 - (int)(T % 100);                                                   // ticks to the next replan step (1 .. 100)
            const int after = ((p.lat_min - 1) / cadence - 1) * cadence;                          // whole rounds an env runs on before its deadline (45 -> 40 ticks)
            reach = std::min(maxleft, (k + after - 1) % 100 + 1);
            if (k <= reach) { r_post = (k + cadence - 1) / cadence + 1; r_free = after / cadence; }
        }
        const int stretch_rounds = (reach + cadence - 1) / cadence + 2;
        if (r_post > 0 && r_post < stretch_rounds) {
            if ((rc = issue_rounds(h, r_post)) || (rc = launch_side_search(h, sw))) return rc;
            const int r2 = std::min(stretch_rounds - r_post, r_free);
            h->dev.b1_small = sw == 4;      // (4-wave search workgroups sit on EVERY CU: what runs beside them must share its LDS and registers)
            rc = issue_rounds(h, r2);
            h->dev.b1_small = false;
            if (rc) return rc;
            HK_HIP(h, hipStreamWaitEvent(h->stream, h->ev_mcts_done, 0));
            rc = issue_rounds(h, stretch_rounds - r_post - r2);
        } else {
            rc = issue_rounds(h, stretch_rounds);
        }
        if (rc) return rc;
        HK_TRY(h, hk::env_flush_mcts(h->dev, h->stream, h->err));
        if ((rc = issue_check(h, true))) return rc;
        HK_HIP(h, hipStreamSynchronize(h->stream));
        maxleft = h->done_host[0];
        if (maxleft <= 0 && !h->done_host[1]) break;
        meter_look(h); apply_meter(h);      // (the copy of this stretch's check is current)
    }
    h->dev.mcts_defer = false;
    h->dev.P.mcts_pause = 0;
    record_schedule(h, p);
    if (maxleft > 0) return fail(h, HK_ERR_HIP, "hk_step: an env did not complete its ticks (internal scheduling error)");
    return HK_OK;
}

// Fixed and lazy calls: the rounds issued up front, then the guard (or, folded, none: the last tick launch is the guard)
static int step_rounds(hk_handle h, const CallPlan& p)
{
    // the rounds every env needs at run_cap ticks a round, then — the laggards packed into the first lane groups — the tail.  With the eager assembly
    // every env retires a cadence per round: there are no laggards to pack, ONE issue (a one-tick call would pay three more GPU operations for the
    // regroup than for its tick; a split call used to join its streams and fork them again for the tail, which left the first stream idle for ~100 us
    // of the driver's 20-tick call)
    const int main_rounds = p.eager ? p.rounds : std::min(p.rounds, (p.n_ticks + p.run_cap - 1) / p.run_cap);
    int rc = issue_rounds(h, main_rounds);
    if (rc) return rc;
    if (p.rounds > main_rounds) {
        if (!p.planner && h->n_policies == 0) {
            HK_TRY(h, hk::env_launch_regroup(h->dev, h->cfg, h->stream, h->err));
        }
        if ((rc = issue_rounds(h, p.rounds - main_rounds))) return rc;
    }
    if (p.t_req >= 0) {
        // this chunk held the replan step: its requests (and nothing older) go to the side stream, in 8-wave workgroups on half the CUs
        if (mcts_join_async(h)) return fail(h, HK_ERR_HIP, "hipStreamWaitEvent (planner side stream)");
        if ((rc = launch_side_search(h, h->tune.mcts_side_waves >= 0 ? h->tune.mcts_side_waves : 8))) return rc;
        // the oldest request in that launch was posted on step T0 + 1 at the earliest: its plan is first used on that step + the smaller latency
        h->mcts_async_deadline = p.T0 + 1 + p.lat_min;
    }
    if (p.planner && !p.short_call) {
        // searches requested in the last rounds of a long call run before it returns
        HK_TRY(h, hk::env_flush_mcts(h->dev, h->stream, h->err));
    }
    if (!p.fold && (rc = issue_check(h, p.lazy))) return rc;
    h->step_pending = p.lazy;
    if (!p.lazy && h->dev.fission && (h->meter_ticks += p.n_ticks) >= METER_TICKS) { h->meter_ticks = 0; if ((rc = meter_copy(h, false))) return rc; }
    record_schedule(h, p);
    if (p.exact_plan) h->opt_pending = true;
    // (the call's plan ends here: the rounds that finish a missed env — verify_optimistic — are plain rounds, none of them skips its solver launch; the
    // fold + skew modes of tests/test_optimistic_plan_gpu.py, round 6)
    h->exact_plan = false;
    h->last_solve_skippable = false;
    h->guard_rounds_left = 0;
    return HK_OK;
}

// n_ticks of every env: settle what the call before left open, plan, apply the plan, issue it
static int step_ticks(hk_handle h, int n_ticks)
{
    meter_look(h);
    const CallPlan p = plan_call(h, n_ticks);
    // the parts of a split call are still open (split_join): only a short folded split call continues them, everything else joins before it puts
    // anything on the handle's stream
    if (h->split_open && !p.continue_split && split_join(h)) return fail(h, HK_ERR_HIP, "hipStreamWaitEvent (the parts of a split call)");
    if (h->mcts_async_deadline >= 0 && (!p.short_call || p.T0 < 0 || p.T0 + n_ticks >= h->mcts_async_deadline) && mcts_join_async(h))
        return fail(h, HK_ERR_HIP, "hipStreamWaitEvent (planner side stream)");
    int rc;
    if (p.planner && h->dev.mcts_ticks > 0 && (!p.short_call || h->dev.mcts_ticks + n_ticks > p.defer || p.t_req >= 0)) {
        if (mcts_join_async(h)) return fail(h, HK_ERR_HIP, "hipStreamWaitEvent (planner side stream)");
        HK_TRY(h, hk::env_flush_mcts(h->dev, h->stream, h->err));
    }
    apply_plan(h, p);
    if (p.fold) h->arm_ticks = n_ticks;
    else HK_TRY(h, hk::env_launch_arm(h->dev, h->cfg, n_ticks, h->stream, h->err));
    return p.pause ? step_pause(h, p) : step_rounds(h, p);
}

// The completion guard of the optimistic fixed-round calls issued since the last look (status bit 2: the last tick launch of a folded call, env_check_kernel
// of the others).  Set: some env did not finish — the belief that the field is in lock-step was wrong (an env finished its race and reset, a time-out) — it
// kept its leftover ticks; the belief is dropped and the laggards are finished as those of a long call are (a guard launch that reports what is left,
// finish_ticks).  Not an error: the state every getter sees afterwards is the state the worst-case schedule would have produced.
static int verify_optimistic(hk_handle h)
{
    h->opt_pending = false;
    int st[4] = {0, 0, 0, 0};
    if (h->dev.P.guard_flag) {
        // the guards raise a pinned host word beside the status bit: nothing to copy back when — as good as always — the plan held (the copy to a pageable
        // buffer was a second round trip behind the stream's completion, ~40 us of a 20-tick call's 820)
        HK_HIP(h, hipStreamSynchronize(h->stream));
        if (__atomic_load_n(h->done_host + 2, __ATOMIC_ACQUIRE) == 0) return HK_OK;
        __atomic_store_n(h->done_host + 2, 0, __ATOMIC_RELEASE);
    }
    HK_HIP(h, hipMemcpyAsync(st, h->dev.status, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    if (!(st[0] & 4)) return HK_OK;
    h->lock_tick = -1;
    hipLaunchKernelGGL(hk::status_and_kernel, dim3(1), dim3(1), 0, h->stream, h->dev.status, ~4);
    HK_HIP(h, hipGetLastError());
    if (h->done_host == nullptr) return fail(h, HK_ERR_HIP, "hk_step: an env did not complete its ticks and the handle has no completion buffer");
    int rc = issue_check(h, true);
    if (rc) return rc;
    h->step_pending = true;
    return finish_ticks(h);
}

// Academy step of a decision tick: CollectObservations -> StackingSensor -> actor -> OnActionReceived latch
static int policy_decide(hk_handle h)
{
    hipEvent_t eo = h->prof.begin(h->stream);
    uint32_t need = 0;                      // only the agents some attached actor drives are observed here
    for (int p = 0; p < h->n_policies; p++)
        for (int j = 0; j < h->policy[p].q.n_slots; j++) need |= 1u << h->policy[p].q.slots[j];
    HK_TRY(h, hk::env_launch_observe(h->dev, h->cfg, need, h->stream, h->err));
    const unsigned long long decision = (unsigned long long)(h->academy_step / h->decision_period);
    const int E = h->cfg.num_envs, A = h->cfg.num_agents;
    // an open rollout: this decision writes row t (hk_rollout.h)
    const auto& ro = h->ro;
    const int t = ro.started;
    const size_t ea = (size_t)E * A;
    for (int p = 0; p < h->n_policies; p++) {
        const hk::PolicyDevice& pd = h->policy[p];
        const int pairs = E * pd.q.n_slots;
        const int w = (int)(decision % (unsigned long long)pd.q.stack);
        if (pd.lq.m > 0) {          // a recurrent actor: its memory is cleared by the stack's own test, before the stack kernel rewrites the epoch word
            hipLaunchKernelGGL(hk::policy_memory_kernel, dim3((pairs + 3) / 4), dim3(256), 0, h->stream, pd.q, pd.lq, E, A, h->dev.envs, h->dev.slot_of,
                               ro.open ? ro.row<float>(HK_RO_MEMORY, t, ea, ro.mem_max) : nullptr, ro.mem_max);
            HK_HIP(h, hipGetLastError());
        }
        hipLaunchKernelGGL(hk::policy_stack_kernel, dim3((pairs + 3) / 4), dim3(256), 0, h->stream, pd.q, E, A, h->dev.envs, h->dev.slot_of,
                           h->dev.obs, w, ro.open ? ro.row<float>(HK_RO_OBS, t, ea, ro.obs_dim) : nullptr, ro.open ? ro.row<int>(HK_RO_FIRST, t, ea) : nullptr);
        HK_HIP(h, hipGetLastError());
    }
    h->prof.end(4, eo, h->stream);
    hk::PolicyRec rec{};
    if (ro.open) {
        rec.steer = ro.row<float>(HK_RO_STEER, t, ea); rec.branch = ro.row<int>(HK_RO_BRANCH, t, ea); rec.raw = ro.row<float>(HK_RO_RAW, t, ea);
        rec.mu = ro.row<float>(HK_RO_MU, t, ea); rec.logits = ro.row<float>(HK_RO_LOGITS, t, ea, ro.nbm); rec.nbm = ro.nbm;
        rec.logp_c = ro.row<float>(HK_RO_LOGP_CONT, t, ea); rec.logp_d = ro.row<float>(HK_RO_LOGP_DISC, t, ea);
    }
    for (int p = 0; p < h->n_policies; p++) {
        const hk::PolicyDevice& pd = h->policy[p];
        const int pairs = E * pd.q.n_slots;
        const int w = (int)(decision % (unsigned long long)pd.q.stack);
        hipEvent_t e = h->prof.begin(h->stream);
        HK_TRY(h, hk::policy_launch_mlp(pd, pairs, pd.q.ring, w, decision, h->cfg.env_id_base, A, nullptr, nullptr, h->dev.act_steer,
                                   h->dev.act_branch, rec, h->stream, h->err));
        h->prof.end(3, e, h->stream);
    }
    if (ro.open) h->ro.started += 1;
    return HK_OK;
}

// the end of an open rollout's interval t: the accumulators into row t, its DONE flags
static int rollout_close_interval(hk_handle h, int t)
{
    const auto& ro = h->ro;
    const int E = h->cfg.num_envs, A = h->cfg.num_agents;
    const size_t ea = (size_t)E * A;
    hipLaunchKernelGGL(hk::rollout_close_kernel, dim3(nblk(ea)), dim3(256), 0, h->stream, h->dev.agents, h->dev.envs, h->dev.slot_of, E, A,
                       ro.driven, ro.row<float>(HK_RO_REWARD, t, ea), ro.row<float>(HK_RO_GROUP_REWARD, t, ea), ro.row<int>(HK_RO_DONE, t, (size_t)E),
                       ro.at<int>(HK_RO_FIELDS), ro.at<int>(HK_RO_FIELDS + 1));
    HK_HIP(h, hipGetLastError());
    h->ro.rows = t + 1;
    return HK_OK;
}

int hk_step(hk_handle h, int n_ticks)
{
    if (int rc = settle(h, SETTLE_STEP)) return rc;
    if (n_ticks < 0) return fail(h, HK_ERR_INVALID, "hk_step: n_ticks < 0");
    if (n_ticks == 0) return HK_OK;
    h->ep.moved = true;                         // (cleared by hk_rollout_close: a step after it ends the episode statistics' carry)
    if (h->n_policies == 0) {
        h->academy_step += n_ticks;
        return step_ticks(h, n_ticks);
    }
    if (h->ro.open) {
        // the decisions this call takes: the multiples of decision_period in [academy_step, academy_step + n_ticks)
        const long long a = h->academy_step, P = h->decision_period;
        const long long decisions = (a + n_ticks - 1) / P - (a + P - 1) / P + 1;
        if (decisions > h->ro.R - h->ro.started)
            return fail(h, HK_ERR_INVALID, "hk_step: the open rollout has " + std::to_string(h->ro.R - h->ro.started) + " rows left, the call takes " +
                                               std::to_string(decisions) + " decisions");
    }
    // with policies attached the Academy steps first in a decision tick; the ticks up to the next decision run fused
    int left = n_ticks;
    while (left > 0) {
        const int phase = (int)(h->academy_step % h->decision_period);
        if (phase == 0) { int rc = policy_decide(h); if (rc) return rc; }
        int chunk = h->decision_period - phase;
        if (chunk > left) chunk = left;
        const bool rec_term = h->ro.open && h->dev.rw.sec_time;       // the terminal rewards of this chunk's resets go to the open row
        if (rec_term) {
            const size_t ea = n_karts(h);
            h->dev.rw.term_step = h->ro.row<float>(HK_RO_TERM_REWARD, h->ro.started - 1, ea);
            h->dev.rw.term_group = h->ro.row<float>(HK_RO_TERM_GROUP_REWARD, h->ro.started - 1, ea);
        }
        int rc = step_ticks(h, chunk);
        h->dev.rw.term_step = nullptr; h->dev.rw.term_group = nullptr;
        if (rc) return rc;
        h->academy_step += chunk;
        left -= chunk;
        if (h->ro.open && h->academy_step % h->decision_period == 0 && (rc = rollout_close_interval(h, h->ro.started - 1))) return rc;
    }
    return HK_OK;
}

int hk_policy_attach(hk_handle h, const hk_policy_desc* desc, const int32_t* agent_slots, int n_slots, int decision_period)
{
    return hk_policy_attach_lstm(h, desc, nullptr, agent_slots, n_slots, decision_period);
}

// lstm == nullptr: hk_policy_attach (every check, message and launch of it)
int hk_policy_attach_lstm(hk_handle h, const hk_policy_desc* desc, const hk_policy_lstm_desc* lstm, const int32_t* agent_slots, int n_slots, int decision_period)
{
    HK_NEED_ENV(h);
    if (h->ro.open) return fail(h, HK_ERR_INVALID, "hk_policy_attach: refused while a rollout is open (hk_rollout_close first)");
    HK_TRY(h, hk::policy_validate(desc, h->err));
    if (lstm) HK_TRY(h, hk::policy_lstm_validate(lstm, h->err));
    if (!agent_slots || n_slots < 1 || n_slots > h->cfg.num_agents || decision_period < 1)
        return fail(h, HK_ERR_INVALID, "hk_policy_attach: bad agent_slots / decision_period");
    if (h->n_policies >= HK_MAX_POLICIES) return fail(h, HK_ERR_INVALID, "hk_policy_attach: HK_MAX_POLICIES policies already attached");
    if (desc->in_dim != hk_obs_dim(h) * desc->stack)
        return fail(h, HK_ERR_INVALID, "hk_policy_attach: in_dim != hk_obs_dim * stack (a model trained for another agent count / horizon)");
    for (int j = 0; j < n_slots; j++) {
        const int a = agent_slots[j];
        if (a < 0 || a >= h->cfg.num_agents || (h->cfg.low_mode[a] != HK_LOW_RL && h->cfg.low_mode[a] != HK_LOW_E2E))
            return fail(h, HK_ERR_INVALID, "hk_policy_attach: agent slot out of range or not LowMode RL / E2E");
        for (int p = 0; p < h->n_policies; p++)
            for (int q = 0; q < h->policy[p].q.n_slots; q++)
                if (h->policy[p].q.slots[q] == a) return fail(h, HK_ERR_INVALID, "hk_policy_attach: agent slot already has a policy");
        for (int q = 0; q < j; q++) if (agent_slots[q] == a) return fail(h, HK_ERR_INVALID, "hk_policy_attach: duplicate agent slot");
    }
    if (h->n_policies > 0 && decision_period != h->decision_period)
        return fail(h, HK_ERR_INVALID, "hk_policy_attach: decision_period differs from the policies already attached (DecisionRequester is per handle)");
    h->ep.moved = true;
    const int idx = h->n_policies;
    int rc = hk::policy_upload(h->policy[idx], desc, idx, hk_obs_dim(h), agent_slots, n_slots, h->cfg.num_envs, h->stream, h->err, lstm ? lstm->memory_size / 2 : 0);
    if (!rc && lstm) rc = hk::policy_lstm_upload(h->policy[idx], lstm, h->cfg.num_envs, h->stream, h->err);
    if (rc) { hk::policy_free(h->policy[idx]); return hand_off(h, rc); }
    h->decision_period = decision_period;
    h->n_policies = idx + 1;
    return idx;
}

// hk_policy_forward (with_mem false: a policy without memory) and hk_policy_forward_mem (with_mem: one with): the staging buffer holds the
// rows' inputs, mu, logits and — with memory — the rows' memory, which the kernel updates in place
static int policy_forward(hk_handle h, const char* fn, bool with_mem, int policy, int rows, const float* obs, const float* mem_in, float* mu, float* logits, float* mem_out)
{
    HK_NEED_ENV(h);
    const std::string f = fn;
    if (policy < 0 || policy >= h->n_policies || rows < 0) return fail(h, HK_ERR_INVALID, f + ": bad policy / rows");
    const hk::PolicyDevice& pd = h->policy[policy];
    if (!with_mem && pd.lq.m > 0) return fail(h, HK_ERR_UNSUPPORTED, f + ": the policy has memory (a recurrent actor): use hk_policy_forward_mem");
    if (with_mem && pd.lq.m == 0) return fail(h, HK_ERR_INVALID, f + ": the policy has no memory (policy: attached without an LSTM): use hk_policy_forward");
    if (rows == 0) return HK_OK;
    if (!obs || !mu || !logits) return fail(h, HK_ERR_INVALID, f + ": NULL pointer");
    const size_t n_in = (size_t)rows * pd.q.in_dim, n_lg = (size_t)rows * pd.q.n_branch, n_mem = (size_t)rows * 2 * pd.lq.m;
    const size_t total = (n_in + rows + n_lg + n_mem) * sizeof(float);
    if (int rc = dev_grow(h, &h->pol_scratch, &h->pol_scratch_bytes, total, total)) return rc;
    float* d_in = (float*)h->pol_scratch;
    float* d_mu = d_in + n_in;
    float* d_lg = d_mu + rows;
    float* d_mem = n_mem ? d_lg + n_lg : nullptr;
    HK_HIP(h, hipMemcpyAsync(d_in, obs, n_in * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (n_mem && mem_in) HK_HIP(h, hipMemcpyAsync(d_mem, mem_in, n_mem * sizeof(float), hipMemcpyHostToDevice, h->stream));
    else if (n_mem) HK_HIP(h, hipMemsetAsync(d_mem, 0, n_mem * sizeof(float), h->stream));
    hipEvent_t e = h->prof.begin(h->stream);
    HK_TRY(h, hk::policy_launch_mlp(pd, rows, d_in, pd.q.stack - 1, 0ull, 0, h->cfg.num_agents, d_mu, d_lg, nullptr, nullptr, hk::PolicyRec{}, h->stream, h->err, d_mem));
    h->prof.end(3, e, h->stream);
    HK_HIP(h, hipMemcpyAsync(mu, d_mu, rows * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipMemcpyAsync(logits, d_lg, n_lg * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (n_mem && mem_out) HK_HIP(h, hipMemcpyAsync(mem_out, d_mem, n_mem * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_policy_forward(hk_handle h, int policy, int rows, const float* obs, float* mu, float* logits)
{
    return policy_forward(h, "hk_policy_forward", false, policy, rows, obs, nullptr, mu, logits, nullptr);
}

int hk_policy_forward_mem(hk_handle h, int policy, int rows, const float* obs, const float* mem_in, float* mu, float* logits, float* mem_out)
{
    return policy_forward(h, "hk_policy_forward_mem", true, policy, rows, obs, mem_in, mu, logits, mem_out);
}

int hk_policy_memory_size(hk_handle h, int policy)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "NULL handle");
    if (policy < 0 || policy >= h->n_policies) return fail(h, HK_ERR_INVALID, "hk_policy_memory_size: bad policy index");
    return 2 * h->policy[policy].lq.m;
}

// hk_policy_memory_get (set false) / hk_policy_memory_set
static int policy_memory_copy(hk_handle h, const char* fn, bool set, int policy, float* mem)
{
    HK_NEED_ENV(h);
    const std::string f = fn;
    if (policy < 0 || policy >= h->n_policies) return fail(h, HK_ERR_INVALID, f + ": bad policy index");
    const hk::PolicyDevice& pd = h->policy[policy];
    if (pd.lq.m == 0) return fail(h, HK_ERR_INVALID, f + ": the policy has no memory (policy: attached without an LSTM)");
    if (!mem) return fail(h, HK_ERR_INVALID, f + ": NULL mem");
    if (set && h->ro.open) return fail(h, HK_ERR_INVALID, f + ": refused while a rollout is open (hk_rollout_close first)");
    const int pairs = h->cfg.num_envs * pd.q.n_slots;
    const size_t bytes = (size_t)pairs * 2 * pd.lq.m * sizeof(float);
    if (set) {
        h->ep.moved = true;
        HK_HIP(h, hipMemcpyAsync(pd.lq.mem, mem, bytes, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(hk::policy_epoch_current_kernel, dim3(nblk(pairs)), dim3(256), 0, h->stream, pd.q, h->cfg.num_envs, h->dev.envs, h->dev.slot_of);
        HK_HIP(h, hipGetLastError());
    } else {
        HK_HIP(h, hipMemcpyAsync(mem, pd.lq.mem, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_policy_memory_get(hk_handle h, int policy, float* mem) { return policy_memory_copy(h, "hk_policy_memory_get", false, policy, mem); }
int hk_policy_memory_set(hk_handle h, int policy, const float* mem) { return policy_memory_copy(h, "hk_policy_memory_set", true, policy, const_cast<float*>(mem)); }

// hk_policy_memory_set of an all-zero array without the host array: a device fill and the same epoch kernel, nothing waited for
int hk_policy_memory_clear(hk_handle h, int policy)
{
    HK_NEED_ENV(h);
    const std::string f = "hk_policy_memory_clear";
    if (policy < 0 || policy >= h->n_policies) return fail(h, HK_ERR_INVALID, f + ": bad policy index");
    const hk::PolicyDevice& pd = h->policy[policy];
    if (pd.lq.m == 0) return fail(h, HK_ERR_INVALID, f + ": the policy has no memory (policy: attached without an LSTM)");
    if (h->ro.open) return fail(h, HK_ERR_INVALID, f + ": refused while a rollout is open (hk_rollout_close first)");
    const int pairs = h->cfg.num_envs * pd.q.n_slots;
    h->ep.moved = true;
    HK_HIP(h, hipMemsetAsync(pd.lq.mem, 0, (size_t)pairs * 2 * pd.lq.m * sizeof(float), h->stream));
    hipLaunchKernelGGL(hk::policy_epoch_current_kernel, dim3(nblk(pairs)), dim3(256), 0, h->stream, pd.q, h->cfg.num_envs, h->dev.envs, h->dev.slot_of);
    HK_HIP(h, hipGetLastError());
    return HK_OK;
}

int hk_policy_set_precision(hk_handle h, int policy, int precision)
{
    HK_NEED_ENV(h);
    if (policy < 0 || policy >= h->n_policies) return fail(h, HK_ERR_INVALID, "hk_policy_set_precision: bad policy index");
    if (precision != HK_POLICY_PREC_F32 && precision != HK_POLICY_PREC_BF16) return fail(h, HK_ERR_INVALID, "hk_policy_set_precision: unknown precision");
    if (h->ro.open) return fail(h, HK_ERR_INVALID, "hk_policy_set_precision: refused while a rollout is open (hk_rollout_close first)");
    hk::PolicyDevice& pd = h->policy[policy];
    if (precision == HK_POLICY_PREC_BF16 && pd.lq.m > 0)
        return fail(h, HK_ERR_UNSUPPORTED, "hk_policy_set_precision: precision HK_POLICY_PREC_BF16 on a policy with memory (the cell has no bf16 form)");
    if (precision == HK_POLICY_PREC_BF16 && !pd.wbf) {
        // the second allocation: every layer's fragment-major bf16 copy, built on the stream from the CURRENT fp32 copies (so after a publish too)
        size_t off[HK_POLICY_MAX_LAYERS + 1] = {};
        for (int l = 0; l < pd.q.n_layers; l++) off[l + 1] = off[l] + hk::policy_bf16_layer_elems(pd.q, l);
        HK_HIP(h, hipMalloc(&pd.wbf, off[pd.q.n_layers] * sizeof(uint16_t)));
        for (int l = 0; l < pd.q.n_layers; l++) pd.bq.Wf[l] = pd.wbf + off[l];
        const hipError_t e = hk::policy_bf16_refresh(pd.q, pd.bq, h->stream);
        if (e != hipSuccess) {
            (void)hipFree(pd.wbf);
            pd.wbf = nullptr;
            pd.bq = hk::PolicyBf16{};
            HK_HIP(h, e);
        }
    }
    pd.prec = precision;
    return HK_OK;
}

int hk_policy_get_precision(hk_handle h, int policy)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "NULL handle");
    if (policy < 0 || policy >= h->n_policies) return fail(h, HK_ERR_INVALID, "hk_policy_get_precision: bad policy index");
    return h->policy[policy].prec;
}

int hk_get_actions(hk_handle h, float* steer, int32_t* branch)
{
    HK_NEED_ENV(h);
    if (!steer || !branch) return fail(h, HK_ERR_INVALID, "hk_get_actions: NULL pointer");
    const size_t cnt = n_karts(h);
    HK_HIP(h, hipMemcpyAsync(steer, h->dev.act_steer, cnt * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipMemcpyAsync(branch, h->dev.act_branch, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

// ------------------------------------------------------------------ rollout recorder (hk.h; device side in hk_rollout.h)
int hk_rollout_begin(hk_handle h, int rows)
{
    HK_NEED_ENV(h);
    if (h->n_policies == 0) return fail(h, HK_ERR_INVALID, "hk_rollout_begin: no actor attached");
    if (h->ro.open) return fail(h, HK_ERR_INVALID, "hk_rollout_begin: a rollout is already open");
    if (rows < 1) return fail(h, HK_ERR_INVALID, "hk_rollout_begin: rows < 1");
    if (h->academy_step % h->decision_period != 0) return fail(h, HK_ERR_INVALID, "hk_rollout_begin: the Academy step is not on a decision (mid-interval)");
    if (!h->cfg.auto_reset) return fail(h, HK_ERR_UNSUPPORTED, "hk_rollout_begin: auto_reset == 0 (an ended episode is parked, never reset)");
    auto& ro = h->ro;
    const int E = h->cfg.num_envs, A = h->cfg.num_agents, D = hk_obs_dim(h);
    int nbm = 1, smax = 1, mem_max = 0;
    uint32_t driven = 0;
    for (int p = 0; p < h->n_policies; p++) {
        mem_max = std::max(mem_max, 2 * h->policy[p].lq.m);
        nbm = std::max(nbm, h->policy[p].q.n_branch);
        smax = std::max(smax, h->policy[p].q.stack);
        for (int j = 0; j < h->policy[p].q.n_slots; j++) driven |= 1u << h->policy[p].q.slots[j];
    }
    const size_t ra = (size_t)rows * E * A, ea = (size_t)E * A;
    size_t elems[HK_RO_FIELDS + 2];
    for (int f = 0; f < HK_RO_FIELDS; f++) elems[f] = ra;
    elems[HK_RO_OBS] = ra * D; elems[HK_RO_LOGITS] = ra * nbm; elems[HK_RO_DONE] = (size_t)rows * E;
    elems[HK_RO_RING0] = ea * (smax - 1) * D; elems[HK_RO_NEXT_OBS] = ea * D;
    elems[HK_RO_MEMORY] = ra * mem_max; elems[HK_RO_NEXT_MEMORY] = ea * mem_max;      // (no recurrent actor: no elements, no bytes)
    elems[HK_RO_FIELDS] = E; elems[HK_RO_FIELDS + 1] = 1;
    size_t off[HK_RO_FIELDS + 2], total = 0;
    for (int f = 0; f < HK_RO_FIELDS + 2; f++) { off[f] = total; total += (elems[f] * 4 + 255) & ~(size_t)255; }
    if (total > ro.bytes) ro.R = 0;          // (a grown buffer holds no rollout until this one's rows are set below)
    if (int rc = dev_grow(h, &ro.buf, &ro.bytes, total, total)) return rc;
    std::memcpy(ro.off, off, sizeof(off));
    ro.R = rows; ro.started = 0; ro.rows = 0; ro.obs_dim = D; ro.nbm = nbm; ro.smax = smax; ro.mem_max = mem_max; ro.driven = driven;
    {   // the episode statistics' carry (hk.h "SELF-PLAY" CARRY): what the statistics of the rollout just closed wrote becomes this one's carry-in
        auto& ep = h->ep;
        bool any = false;
        for (int p = 0; p < HK_MAX_POLICIES; p++) {
            ep.carry_ok[p] = ep.buf && !ep.moved && ro.gen > 0 && p < ro.npol && ep.stats_gen[p] == ro.gen;
            any = any || ep.carry_ok[p];
        }
        if (any) ep.in ^= 1;
    }
    ro.gen += 1; ro.npol = h->n_policies;
    HK_HIP(h, hipMemsetAsync(ro.buf, 0, total, h->stream));
    const unsigned long long decision = (unsigned long long)(h->academy_step / h->decision_period);
    for (int p = 0; p < h->n_policies; p++) {
        const hk::PolicyParams& q = h->policy[p].q;
        const size_t n = (size_t)E * q.n_slots * (q.stack - 1) * D;
        if (n == 0) continue;
        hipLaunchKernelGGL(hk::rollout_ring0_kernel, dim3(nblk(n)), dim3(256), 0, h->stream, q, E, A, (int)(decision % (unsigned long long)q.stack),
                           smax, ro.at<float>(HK_RO_RING0));
        HK_HIP(h, hipGetLastError());
    }
    hipLaunchKernelGGL(hk::rollout_epoch_kernel, dim3(nblk(E)), dim3(256), 0, h->stream, h->dev.envs, h->dev.slot_of, E, ro.at<int>(HK_RO_FIELDS));
    HK_HIP(h, hipGetLastError());
    ro.open = true;
    return HK_OK;
}

int hk_rollout_rows(hk_handle h)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "NULL handle");
    return h->ro.rows;
}

int hk_rollout_close(hk_handle h)
{
    HK_NEED_ENV(h);
    auto& ro = h->ro;
    if (!ro.open) return fail(h, HK_ERR_INVALID, "hk_rollout_close: no rollout is open");
    if (h->academy_step % h->decision_period != 0) return fail(h, HK_ERR_INVALID, "hk_rollout_close: mid-interval (step to the next decision first)");
    // the bootstrap observation: the observe kernel without its reward events, so that the next decision raises them as usual
    HK_TRY(h, hk::env_launch_observe_quiet(h->dev, h->cfg, ro.driven, ro.at<float>(HK_RO_NEXT_OBS), h->stream, h->err));
    // the bootstrap memory of the recurrent actors: what the last completed row left, zero where its interval ended the episode
    for (int p = 0; p < h->n_policies && ro.mem_max > 0; p++) {
        const hk::PolicyDevice& pd = h->policy[p];
        if (pd.lq.m == 0) continue;
        const int E = h->cfg.num_envs;
        const size_t n = (size_t)E * pd.q.n_slots * 2 * pd.lq.m;
        hipLaunchKernelGGL(hk::rollout_next_memory_kernel, dim3(nblk(n)), dim3(256), 0, h->stream, pd.q, pd.lq, E, h->cfg.num_agents,
                           ro.rows > 0 ? ro.row<int>(HK_RO_DONE, ro.rows - 1, (size_t)E) : nullptr, ro.at<float>(HK_RO_NEXT_MEMORY), ro.mem_max);
        HK_HIP(h, hipGetLastError());
    }
    ro.open = false;
    h->ep.moved = false;
    int bad = 0;
    HK_HIP(h, hipMemcpyAsync(&bad, ro.at<int>(HK_RO_FIELDS + 1), sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    if (bad) return fail(h, HK_ERR_INVALID, "hk_rollout_close: an env ended more than one episode inside one decision interval; the rows cannot express it");
    return HK_OK;
}

void* hk_rollout_ptr(hk_handle h, int field)
{
    if (!h) { fail(nullptr, HK_ERR_INVALID, "NULL handle"); return nullptr; }
    if (field < 0 || field >= HK_RO_FIELDS) { fail(h, HK_ERR_INVALID, "hk_rollout_ptr: bad field"); return nullptr; }
    if (!h->ro.buf || h->ro.R == 0) { fail(h, HK_ERR_INVALID, "hk_rollout_ptr: no rollout yet (hk_rollout_begin)"); return nullptr; }
    if ((field == HK_RO_MEMORY || field == HK_RO_NEXT_MEMORY) && h->ro.mem_max == 0) {
        fail(h, HK_ERR_INVALID, "hk_rollout_ptr: field MEMORY / NEXT_MEMORY has no elements (the rollout has no recurrent actor)");
        return nullptr;
    }
    return h->ro.at<void>(field);
}

// ------------------------------------------------------------------ PPO trainer (hk.h; device side in hk_ppo.h)
extern "C++" {
namespace {

// The two precisions (hk.h "PRECISION") share every line from the gather to Adam: a trunk matrix is a PpoMat, and ppo_gather, ppo_product
// (ppo_wgrad goes through it), ppo_colsum, ppo_head_back and ppo_weights are the only places that look at which kind it is.

// a matrix in the trainer's trunk precision: fp32 (f) or bf16 bit patterns (b), exactly one of them set
struct PpoMat {
    float* f = nullptr;
    uint16_t* b = nullptr;
    PpoMat() = default;
    PpoMat(float* p) : f(p) {}
    PpoMat(uint16_t* p) : b(p) {}
};

// the minibatch workspace of a trainer at capacity M rows: pointers into one allocation (Ppo::ws)
struct PpoWs {
    int* ids; int* valid; int* n_valid;
    // HK_PPO_PREC_BF16: the input, the post-activations below the last layer and the deltas are bf16; the last layer's stays fp32 (the heads read it)
    PpoMat X0;
    float* Za[HK_POLICY_MAX_LAYERS]; PpoMat Aa[HK_POLICY_MAX_LAYERS];
    float* Zc[HK_POLICY_MAX_LAYERS]; PpoMat Ac[HK_POLICY_MAX_LAYERS];
    PpoMat d0, d1;
    float *dhead, *dls, *dv, *part, *stats;
    double *rowstat, *acc;
    float *mb_mu, *mb_logits, *mb_v;
};

// one allocation handed out front to back in 256-byte steps (base nullptr: only the size is wanted)
struct PpoBump {
    char* base;
    size_t off = 0;
    char* take(size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; }
};

size_t ppo_ws_layout(const hk_context::Ppo& t, int M, PpoWs* w)
{
    PpoBump a{w ? (char*)t.ws : nullptr};
    const bool bf = t.prec == HK_PPO_PREC_BF16;
    auto mat = [&](size_t count, bool bits) { char* p = a.take(count * (bits ? 2 : 4)); return bits ? PpoMat((uint16_t*)p) : PpoMat((float*)p); };
    auto fl = [&](size_t count) { return (float*)a.take(count * 4); };
    const size_t Mz = (size_t)M;
    const int Ha = t.actor.hidden, Hc = t.critic.hidden, Hm = std::max(Ha, Hc), in = t.actor.in_dim, nb = t.actor.n_branch;
    size_t mn = (size_t)(1 + nb) * Ha;                          // the largest weight gradient: a layer's H x K, or the heads'
    mn = std::max(mn, (size_t)Ha * std::max(in, Ha));
    mn = std::max(mn, (size_t)Hc * std::max(in, Hc));
    const size_t nz = (Mz + hk::PPO_KCH - 1) / hk::PPO_KCH;
    PpoWs d{};
    d.ids = (int*)a.take(Mz * 4); d.valid = (int*)a.take(Mz * 4); d.n_valid = (int*)a.take(16);
    d.X0 = mat(Mz * in, bf);
    for (int l = 0; l < t.actor.n_layers; l++) { d.Za[l] = fl(Mz * Ha); d.Aa[l] = mat(Mz * Ha, bf && l < t.actor.n_layers - 1); }
    for (int l = 0; l < t.critic.n_layers; l++) { d.Zc[l] = fl(Mz * Hc); d.Ac[l] = mat(Mz * Hc, bf && l < t.critic.n_layers - 1); }
    d.d0 = mat(Mz * Hm, bf); d.d1 = mat(Mz * Hm, bf);
    d.dhead = fl(Mz * hk::PM_MAX_OUT); d.dls = fl(Mz); d.dv = fl(Mz);
    d.part = fl(nz * mn);
    d.stats = fl(8);
    d.rowstat = (double*)a.take(Mz * 6 * 8); d.acc = (double*)a.take(8 * 8);
    d.mb_mu = fl(Mz); d.mb_logits = fl(Mz * nb); d.mb_v = fl(Mz);
    if (w) *w = d;
    return a.off;
}

// the workspace as it is allocated now
PpoWs ppo_ws(const hk_context::Ppo& t) { PpoWs w; ppo_ws_layout(t, t.cap, &w); return w; }

int ppo_ensure_ws(hk_handle h, hk_context::Ppo& t, int M, PpoWs& w)
{
    if (M > t.cap) {
        t.last_m = 0;
        if (int rc = dev_grow(h, &t.ws, &t.cap, M, ppo_ws_layout(t, M, nullptr))) return rc;
    }
    w = ppo_ws(t);
    return HK_OK;
}

// the rows' buffer of a trainer (Ppo::rowbuf) after hk_ppo_advantages set t.n: V_OLD, ADV, RET [n], V_BOOT [E S], PERM [n]
struct PpoRowBuf { float *v_old, *adv, *ret, *v_boot; int* perm; };
PpoRowBuf ppo_rowbuf(hk_handle h, const hk_context::Ppo& t)
{
    const size_t n = (size_t)t.n, nbt = (size_t)h->cfg.num_envs * h->policy[t.policy].q.n_slots;
    float* p = t.rowbuf;
    return PpoRowBuf{p, p + n, p + 2 * n, p + 3 * n, (int*)(p + 3 * n + nbt)};
}

hk::PpoRows ppo_rows(hk_handle h, const hk_context::Ppo& t)
{
    const auto& ro = h->ro;
    const hk::PolicyParams& q = h->policy[t.policy].q;
    hk::PpoRows P{};
    P.obs = ro.at<float>(HK_RO_OBS); P.ring0 = ro.at<float>(HK_RO_RING0); P.next_obs = ro.at<float>(HK_RO_NEXT_OBS);
    P.raw = ro.at<float>(HK_RO_RAW); P.reward = ro.at<float>(HK_RO_REWARD); P.term_reward = ro.at<float>(HK_RO_TERM_REWARD);
    P.logp_c = ro.at<float>(HK_RO_LOGP_CONT); P.logp_d = ro.at<float>(HK_RO_LOGP_DISC);
    P.first = ro.at<int>(HK_RO_FIRST); P.branch = ro.at<int>(HK_RO_BRANCH); P.done = ro.at<int>(HK_RO_DONE);
    P.mean = q.mean; P.std = q.std;
    P.R = ro.rows; P.E = h->cfg.num_envs;        // the completed rows: a rollout may close before all R rows of hk_rollout_begin
    P.A = h->cfg.num_agents; P.S = q.n_slots; P.D = ro.obs_dim; P.stack = q.stack; P.smax = ro.smax;
    P.in_dim = q.in_dim; P.normalize = q.normalize;
    for (int j = 0; j < HK_MAX_AGENTS; j++) P.slots[j] = q.slots[j];
    return P;
}

void ppo_gather(hipStream_t s, const hk::PpoRows& P, const int* ids, int m, int boot, PpoMat X0, int* valid)
{
    const dim3 grid(nblk((size_t)m * P.in_dim));
    if (X0.b) hipLaunchKernelGGL(hk::ppo_gather_kernel<uint16_t>, grid, dim3(256), 0, s, P, ids, m, boot, X0.b, valid);
    else hipLaunchKernelGGL(hk::ppo_gather_kernel<float>, grid, dim3(256), 0, s, P, ids, m, boot, X0.f, valid);
}

// C [M][N] = epilogue EPI of the product of A and B over K, in chunks of kch (hk_ppo.h).  An operand is given as its leading dimension and
// whether k is its contiguous index — the bf16 kernel's form, which the fp32 kernel's two strides per operand follow from
template <int EPI>
void ppo_product(hipStream_t s, int M, int N, int K, PpoMat A, int lda, bool a_kc, PpoMat B, int ldb, bool b_kc, const float* bias, PpoMat C, int ldc, float* Z,
                 int kch)
{
    const int nz = (K + kch - 1) / kch;
    const unsigned gz = nz < 1 ? 1 : nz;
    if (A.b)
        hipLaunchKernelGGL(hk::ppo_gemm_bf16_kernel<EPI>, dim3(nblk(N, hk::PB_TN), nblk(M, hk::PB_TM), gz), dim3(256), 0, s, M, N, K, A.b, lda, (int)a_kc, B.b,
                           ldb, (int)b_kc, bias, C.f, C.b, ldc, Z, kch);
    else
        hipLaunchKernelGGL(hk::ppo_gemm_kernel<EPI>, dim3(nblk(N, hk::PPO_TN), nblk(M, hk::PPO_TM), gz), dim3(256), 0, s, M, N, K, A.f, a_kc ? lda : 1,
                           a_kc ? 1 : lda, B.f, b_kc ? 1 : ldb, b_kc ? ldb : 1, bias, C.f, ldc, Z, kch);
}

// a weight gradient out [M][N] = sum over the m rows of D[i][o] X[i][c] (both row-major, of one kind): fixed chunks of PPO_KCH rows into part,
// the partial tiles combined in chunk order (out1: the rows from the second on go there, the heads' W_branch)
void ppo_wgrad(hipStream_t s, float* part, int M, int N, int m, PpoMat D, int ldd, PpoMat X, int ldx, float* out0, float* out1)
{
    const int nz = (m + hk::PPO_KCH - 1) / hk::PPO_KCH;
    ppo_product<0>(s, M, N, m, D, ldd, false, X, ldx, false, nullptr, part, N, nullptr, hk::PPO_KCH);
    hipLaunchKernelGGL(hk::ppo_combine_kernel, dim3(nblk((size_t)M * N)), dim3(256), 0, s, part, nz, M, N, out0, out1);
}

void ppo_colsum(hipStream_t s, PpoMat X, int m, int ld, int ncol, float* out)
{
    if (X.b) hipLaunchKernelGGL(hk::ppo_colsum_kernel<hk::ppo_bf16>, dim3(ncol), dim3(256), 0, s, reinterpret_cast<const hk::ppo_bf16*>(X.b), m, ld, out);
    else hipLaunchKernelGGL(hk::ppo_colsum_kernel<float>, dim3(ncol), dim3(256), 0, s, X.f, m, ld, out);
}

// the last trunk layer's delta dA = (dhead [W0; W1]) * swish'(Z), through the heads' weights on the vector ALU
void ppo_head_back(hipStream_t s, int m, int H, int n_out, const float* dhead, int ldd, const float* W0, const float* W1, const float* Z, PpoMat dA)
{
    const dim3 grid(nblk((size_t)m * H));
    if (dA.b) hipLaunchKernelGGL(hk::ppo_head_back_bf16_kernel, grid, dim3(256), 0, s, m, H, n_out, dhead, ldd, W0, W1, Z, dA.b);
    else hipLaunchKernelGGL(hk::ppo_head_back_kernel, grid, dim3(256), 0, s, m, H, n_out, dhead, ldd, W0, W1, Z, dA.f);
}

// the weight at PARAMS offset o as the trunk products read it: PARAMS, or their bf16 shadow (what follows the actor shadow_pad elements on)
PpoMat ppo_weights(const hk_context::Ppo& t, size_t o)
{
    if (t.prec != HK_PPO_PREC_BF16) return t.param + o;
    return t.shadow + o + (o >= t.actor.count ? t.shadow_pad : 0);
}

// HK_PPO_PREC_BF16: PARAMS rounded into the shadow — after Adam, and at every entry point, since PARAMS is writable through hk_ppo_ptr
void ppo_shadow_refresh(hipStream_t s, const hk_context::Ppo& t)
{
    if (t.prec != HK_PPO_PREC_BF16) return;
    hipLaunchKernelGGL(hk::ppo_shadow_kernel, dim3(nblk(t.P)), dim3(256), 0, s, t.param, t.shadow, t.P, t.actor.count, t.shadow_pad);
}

// The trunk functions serve a PpoNet and the POCA critic's encoder (hk::PocaNet's oW / ob, n_layers layers of hidden x hidden on the pooled
// sequences): what a trunk's first layer reads
inline int ppo_trunk_in(const hk::PpoNet& net) { return net.in_dim; }
inline int ppo_trunk_in(const hk::PocaNet& net) { return net.hidden; }

// trunk forward on X0: Z[l] = W_l a_{l-1} + b_l (MFMA, k ascending; fp32), A[l] = swish(Z[l]) in the kind the workspace gave it
template <typename Net>
void ppo_trunk_forward(hipStream_t s, const hk_context::Ppo& t, const Net& net, PpoMat X0, int m, float* const* Z, const PpoMat* A)
{
    const int H = net.hidden;
    for (int l = 0; l < net.n_layers; l++) {
        const int K = l == 0 ? ppo_trunk_in(net) : H;
        ppo_product<1>(s, m, H, K, l == 0 ? X0 : A[l - 1], K, true, ppo_weights(t, net.oW[l]), K, true, t.param + net.ob[l], A[l], H, Z[l], K);
    }
}

// trunk backward from dcur = dL / dZ[L - 1]: weight and bias gradients into GRAD (through part), delta through W_l * swish' (dnext: the other
// delta buffer; one swap per layer above the first).  -> the buffer that holds dL / dZ[0]
template <typename Net>
PpoMat ppo_trunk_backward(hipStream_t s, const hk_context::Ppo& t, const Net& net, float* part, PpoMat X0, int m, float* const* Z, const PpoMat* A, PpoMat dcur,
                          PpoMat dnext)
{
    const int H = net.hidden;
    float* grad = t.param + t.P;
    for (int l = net.n_layers - 1; l >= 0; l--) {
        const int K = l == 0 ? ppo_trunk_in(net) : H;
        ppo_wgrad(s, part, H, K, m, dcur, H, l == 0 ? X0 : A[l - 1], K, grad + net.oW[l], nullptr);
        ppo_colsum(s, dcur, m, H, H, grad + net.ob[l]);
        if (l > 0) {
            ppo_product<2>(s, m, H, H, dcur, H, true, ppo_weights(t, net.oW[l]), H, false, nullptr, dnext, H, Z[l - 1], H);
            std::swap(dcur, dnext);
        }
    }
    return dcur;
}

// a value head's backward (W, b at PARAMS offsets oW, ob; H wide under the last activations A of pre-activations Z): the delta dv [m] into d0 = dL / dZ,
// and the head's gradients
void ppo_value_head_back(hipStream_t s, const hk_context::Ppo& t, float* part, int m, int H, float* dv, size_t oW, size_t ob, const float* Z, PpoMat A, PpoMat d0)
{
    float* grad = t.param + t.P;
    ppo_head_back(s, m, H, 1, dv, 1, t.param + oW, nullptr, Z, d0);
    ppo_wgrad(s, part, 1, H, m, dv, 1, A, H, grad + oW, nullptr);
    ppo_colsum(s, dv, m, 1, 1, grad + ob);
}

// What differs between the trainers under ppo_loss_kernel: what stands in for the critic's last activation [m][Hc], the value head, the row ids
struct PpoValueIn { const float* Ac; int Hc; const float *W_v, *b_v; const int* ids; };

// the actor half of a minibatch, first part: ppo_loss_kernel and the stats kernel on what the heads read — Aa [m][Ha], the trunk's last
// activations or a recurrent actor's h' (t.actor's head offsets are the m-wide heads' then) — and the value input c (acc: into the update's
// stats accumulator too).  sids: a recurrent minibatch's ms sequence ids, whose stats count skipped SEQUENCES
void ppo_actor_loss(hk_handle h, const hk_context::Ppo& t, const hk::PpoRows& P, const PpoWs& w, const float* Aa, int Ha, const PpoValueIn& c, int m, float eps,
                    float beta, bool acc, const int32_t* sids = nullptr, int ms = 0)
{
    const PpoRowBuf rows = ppo_rowbuf(h, t);
    const float* prm = t.param;
    const hk::PpoNet& na = t.actor;
    hk::PpoLossArgs L{};
    L.Aa = Aa; L.Ac = c.Ac;
    L.W_mu = prm + na.oWmu; L.b_mu = prm + na.obmu; L.log_sigma = prm + na.ols; L.W_br = prm + na.oWbr; L.b_br = prm + na.obbr;
    L.W_v = c.W_v; L.b_v = c.b_v;
    L.v_old = rows.v_old; L.adv = rows.adv; L.ret = rows.ret;
    L.ids = c.ids; L.valid = w.valid; L.n_valid = w.n_valid; L.m = m; L.n = t.n; L.Ha = Ha; L.Hc = c.Hc; L.nb = na.n_branch;
    L.eps = eps; L.beta = beta;
    L.dhead = w.dhead; L.dls = w.dls; L.dv = w.dv; L.rowstat = w.rowstat;
    L.mu_out = w.mb_mu; L.logit_out = w.mb_logits; L.v_out = w.mb_v;
    hipLaunchKernelGGL(hk::ppo_loss_kernel, dim3(nblk(m)), dim3(256), 0, h->stream, P, L);
    if (sids) hipLaunchKernelGGL(hk::ppo_lstm_stats_kernel, dim3(1), dim3(256), 0, h->stream, w.rowstat, m, sids, ms, t.n_seq, w.stats, acc ? w.acc : nullptr);
    else hipLaunchKernelGGL(hk::ppo_stats_kernel, dim3(1), dim3(256), 0, h->stream, w.rowstat, m, w.stats, acc ? w.acc : nullptr);
}

// the gradients of the actor's heads (fp32 in both precisions) on what they read, A [m][H]: W_mu / W_branch through part, the biases and log_sigma
void ppo_head_grads(hipStream_t s, const hk_context::Ppo& t, float* part, const PpoWs& w, int m, int H, PpoMat A)
{
    float* grad = t.param + t.P;
    const hk::PpoNet& na = t.actor;
    ppo_wgrad(s, part, 1 + na.n_branch, H, m, w.dhead, hk::PM_MAX_OUT, A, H, grad + na.oWmu, grad + na.oWbr);
    ppo_colsum(s, w.dhead, m, hk::PM_MAX_OUT, 1, grad + na.obmu);
    ppo_colsum(s, w.dhead + 1, m, hk::PM_MAX_OUT, na.n_branch, grad + na.obbr);
    ppo_colsum(s, w.dls, m, 1, 1, grad + na.ols);
}

// ... second part: the heads' backward (vector ALU), then the trunk's
void ppo_actor_backward(hipStream_t s, const hk_context::Ppo& t, const PpoWs& w, int m)
{
    const float* prm = t.param;
    const hk::PpoNet& na = t.actor;
    const int Ha = na.hidden, La = na.n_layers - 1;
    ppo_head_back(s, m, Ha, 1 + na.n_branch, w.dhead, hk::PM_MAX_OUT, prm + na.oWmu, prm + na.oWbr, w.Za[La], w.d0);
    ppo_head_grads(s, t, w.part, w, m, Ha, w.Aa[La]);
    ppo_trunk_backward(s, t, na, w.part, w.X0, m, w.Za, w.Aa, w.d0, w.d1);
}

// ---- POCA (hk.h "POCA"; device side in hk_poca.h).  Everything below is reached only through a trainer made by hk_ppo_create_poca.

// the POCA workspace at a capacity of G groups: m = G S agent rows, E2 = 2 m entities, NS = (S + 1) G sequences, SR = NS S sequence rows
struct PocaWs {
    int *gids, *rid;
    float *XA, *Zent, *U, *N, *Q, *K, *V, *C, *alpha, *Oz, *O, *Zp;
    float2 *estat, *ostat;
    float* Ze[HK_POLICY_MAX_LAYERS]; PpoMat Ae[HK_POLICY_MAX_LAYERS];          // the encoder, as the trunk functions take it (always fp32)
    float *out, *vrow, *brow, *mb_v, *dout, *d0, *d1, *dZp, *dPre, *dC, *dQs, *dKs, *dVs, *dQ, *dK, *dV, *dR, *dNq, *dNk, *dNv, *dZent, *part;
    double *rowstat_b, *pacc;
    float *pstats, *consts;          // consts: {1.0f, 0.0f}
};

size_t poca_ws_layout(const hk_context::Ppo& t, int S, int G, PocaWs* w)
{
    PpoBump a{w ? (char*)t.pws : nullptr};
    auto fl = [&](size_t count) { return (float*)a.take(count * 4); };
    const hk::PocaNet& pn = t.pnet;
    const size_t H = pn.hidden, m = (size_t)G * S, E2 = 2 * m, NS = (size_t)(S + 1) * G, SR = NS * S;
    PocaWs d{};
    d.gids = (int*)a.take((size_t)G * 4); d.rid = (int*)a.take(m * 4);
    d.XA = fl(m * pn.n_act);
    d.Zent = fl(E2 * H); d.U = fl(E2 * H); d.N = fl(E2 * H); d.Q = fl(E2 * H); d.K = fl(E2 * H); d.V = fl(E2 * H);
    d.C = fl(SR * H); d.alpha = fl(NS * hk::POCA_HEADS * hk::POCA_MAXS * hk::POCA_MAXS); d.Oz = fl(SR * H); d.O = fl(SR * H); d.Zp = fl(NS * H);
    d.estat = (float2*)a.take(E2 * 8); d.ostat = (float2*)a.take(SR * 8);
    for (int l = 0; l < pn.n_layers; l++) { d.Ze[l] = fl(NS * H); d.Ae[l] = fl(NS * H); }
    d.out = fl(NS); d.vrow = fl(m); d.brow = fl(m); d.mb_v = fl(G); d.dout = fl(NS);
    d.d0 = fl(NS * H); d.d1 = fl(NS * H); d.dZp = fl(NS * H);
    d.dPre = fl(SR * H); d.dC = fl(SR * H); d.dQs = fl(SR * H); d.dKs = fl(SR * H); d.dVs = fl(SR * H);
    d.dQ = fl(E2 * H); d.dK = fl(E2 * H); d.dV = fl(E2 * H); d.dR = fl(E2 * H); d.dNq = fl(E2 * H); d.dNk = fl(E2 * H); d.dNv = fl(E2 * H); d.dZent = fl(E2 * H);
    const size_t nz = (std::max(SR, E2) + hk::PPO_KCH - 1) / hk::PPO_KCH;          // the longest weight gradient's chunks, the largest one's tile
    d.part = fl(nz * H * std::max((size_t)pn.n_act, H));
    d.rowstat_b = (double*)a.take(m * 8); d.pacc = (double*)a.take(2 * 8);
    d.pstats = fl(HK_POCA_STATS); d.consts = fl(2);
    if (w) *w = d;
    return a.off;
}

// the workspace as it is allocated now
PocaWs poca_ws(hk_handle h, const hk_context::Ppo& t) { PocaWs pw; poca_ws_layout(t, h->policy[t.policy].q.n_slots, t.pcap, &pw); return pw; }

int poca_ensure_ws(hk_handle h, hk_context::Ppo& t, int G, PocaWs& w)
{
    if (G > t.pcap) {
        t.last_mg = 0;
        if (int rc = dev_grow(h, &t.pws, &t.pcap, G, poca_ws_layout(t, h->policy[t.policy].q.n_slots, G, nullptr))) return rc;
        w = poca_ws(h, t);
        const float c[2] = {1.0f, 0.0f};
        HK_HIP(h, hipMemcpyAsync(w.consts, c, sizeof(c), hipMemcpyHostToDevice, h->stream));
        HK_HIP(h, hipMemsetAsync(w.pacc, 0, 2 * sizeof(double), h->stream));
        HK_HIP(h, hipStreamSynchronize(h->stream));          // (c is on this frame)
    }
    w = poca_ws(h, t);
    return HK_OK;
}

// the rows' extra buffer of a POCA trainer: B_OLD, TEAM_REWARD [n]
struct PocaRowBuf { float *b_old, *team; };
PocaRowBuf poca_rowbuf(const hk_context::Ppo& t) { return PocaRowBuf{t.prow, t.prow + t.n}; }

// a plain fp32 product C [M][N] = EPI(A [M][K] B^T + bias), B [N][K] (a weight as stored) ...
template <int EPI>
void poca_lin(hipStream_t s, int M, int N, int K, const float* A, const float* W, const float* bias, float* C, float* Z)
{
    ppo_product<EPI>(s, M, N, K, PpoMat(const_cast<float*>(A)), K, true, PpoMat(const_cast<float*>(W)), K, true, bias, PpoMat(C), N, Z, K);
}
// ... and C [M][N] = EPI(A [M][K] B), B [K][N]: a delta through a weight
template <int EPI>
void poca_lin_t(hipStream_t s, int M, int N, int K, const float* A, const float* W, float* C, float* Z)
{
    ppo_product<EPI>(s, M, N, K, PpoMat(const_cast<float*>(A)), K, true, PpoMat(const_cast<float*>(W)), N, false, nullptr, PpoMat(C), N, Z, K);
}

// the critic's forward over the groups gids[0 .. mg): gather (X0, valid of the PPO workspace w), embeddings, attention, encoder, the head -> pw.out [NS]
void poca_forward(hipStream_t s, const hk_context::Ppo& t, const hk::PpoRows& P, const PpoWs& w, const PocaWs& pw, const int* gids, int mg, int boot)
{
    const hk::PocaNet& pn = t.pnet;
    const float* prm = t.param;
    const int S = P.S, H = pn.hidden, in = pn.in_dim, na = pn.n_act, m = mg * S, E2 = 2 * m, NS = (S + 1) * mg, SR = NS * S;
    hipLaunchKernelGGL(hk::poca_rows_kernel, dim3(nblk(m)), dim3(256), 0, s, gids, mg, S, P.R * P.E, P.E, boot, pw.rid);
    ppo_gather(s, P, pw.rid, m, boot, w.X0, w.valid);
    hipLaunchKernelGGL(hk::poca_actfeat_kernel, dim3(nblk((size_t)m * na)), dim3(256), 0, s, P, pw.rid, m, w.X0.f, pw.XA, pn.n_branch);
    poca_lin<1>(s, m, H, in, w.X0.f, prm + pn.oWobs, prm + pn.obobs, pw.U, pw.Zent);
    poca_lin<1>(s, m, H, na, pw.XA, prm + pn.oWact, prm + pn.obact, pw.U + (size_t)m * H, pw.Zent + (size_t)m * H);
    hipLaunchKernelGGL(hk::poca_ln_kernel<false>, dim3(nblk(E2, 4)), dim3(256), 0, s, pw.U, nullptr, E2, H, S, m, pw.N, pw.estat);
    poca_lin<0>(s, E2, H, H, pw.N, prm + pn.oWq, prm + pn.obq, pw.Q, nullptr);
    poca_lin<0>(s, E2, H, H, pw.N, prm + pn.oWk, prm + pn.obk, pw.K, nullptr);
    poca_lin<0>(s, E2, H, H, pw.N, prm + pn.oWv, prm + pn.obv, pw.V, nullptr);
    hipLaunchKernelGGL(hk::poca_attn_fwd_kernel, dim3(nblk(NS, 4)), dim3(256), 0, s, pw.Q, pw.K, pw.V, NS, S, m, H, pw.C, pw.alpha);
    poca_lin<0>(s, SR, H, H, pw.C, prm + pn.oWout, prm + pn.obout, pw.Oz, nullptr);
    hipLaunchKernelGGL(hk::poca_ln_kernel<true>, dim3(nblk(SR, 4)), dim3(256), 0, s, pw.Oz, pw.N, SR, H, S, m, pw.O, pw.ostat);
    hipLaunchKernelGGL(hk::poca_pool_kernel, dim3(nblk((size_t)NS * H)), dim3(256), 0, s, pw.O, NS, S, H, pw.Zp);
    ppo_trunk_forward(s, t, pn, pw.Zp, NS, pw.Ze, pw.Ae);
    hipLaunchKernelGGL(hk::poca_value_kernel, dim3(nblk(NS)), dim3(256), 0, s, pw.Ae[pn.n_layers - 1].f, NS, H, prm + pn.owval, prm + pn.obval, pw.out);
}

// one POCA minibatch of mg group ids: the actor side is ppo_mb's (ppo_actor_loss, ppo_actor_backward); the critic side is the attention critic
int poca_mb(hk_handle h, hk_context::Ppo& t, const int32_t* gids, int mg, float eps, float beta, bool acc)
{
    const hk::PpoRows P = ppo_rows(h, t);
    const int S = P.S, m = mg * S;
    PpoWs w;
    PocaWs pw;
    int rc = ppo_ensure_ws(h, t, m, w);
    if (rc) return rc;
    if ((rc = poca_ensure_ws(h, t, mg, pw))) return rc;
    hipStream_t s = h->stream;
    const PpoRowBuf rows = ppo_rowbuf(h, t);
    const PocaRowBuf prows = poca_rowbuf(t);
    const float* prm = t.param;
    float* grad = t.param + t.P;
    const hk::PocaNet& pn = t.pnet;
    const int H = pn.hidden, L = pn.n_layers;
    const int E2 = 2 * m, NS = (S + 1) * mg, SR = NS * S;
    poca_forward(s, t, P, w, pw, gids, mg, 0);
    hipLaunchKernelGGL(hk::poca_scatter_kernel, dim3(nblk(m)), dim3(256), 0, s, pw.out, pw.rid, m, S, t.n, 0, nullptr, nullptr, nullptr, pw.vrow, pw.brow, pw.mb_v);
    hipLaunchKernelGGL(hk::ppo_count_kernel, dim3(1), dim3(256), 0, s, w.valid, m, w.n_valid);
    ppo_trunk_forward(s, t, t.actor, w.X0, m, w.Za, w.Aa);
    // ppo_loss_kernel as it is: its "critic activation" is the row's group value, one wide, under the head (1, 0), so v = fmaf(V, 1, 0) = V
    ppo_actor_loss(h, t, P, w, w.Aa[t.actor.n_layers - 1].f, t.actor.hidden, PpoValueIn{pw.vrow, 1, pw.consts, pw.consts + 1, pw.rid}, m, eps, beta, acc);
    hipLaunchKernelGGL(hk::poca_loss_kernel, dim3(nblk(mg)), dim3(256), 0, s, pw.brow, pw.rid, w.valid, w.n_valid, prows.b_old, rows.ret, w.dv, mg, S, t.n, eps,
                       pw.dout, pw.rowstat_b);
    hipLaunchKernelGGL(hk::poca_stats_kernel, dim3(1), dim3(256), 0, s, pw.rowstat_b, m, S, w.n_valid, w.stats, acc ? w.acc : nullptr, pw.pstats,
                       acc ? pw.pacc : nullptr);
    ppo_actor_backward(s, t, w, m);
    // critic: the head and the encoder over the NS sequences, then the encoder's input
    ppo_value_head_back(s, t, pw.part, NS, H, pw.dout, pn.owval, pn.obval, pw.Ze[L - 1], pw.Ae[L - 1], pw.d0);
    const PpoMat dz0 = ppo_trunk_backward(s, t, pn, pw.part, pw.Zp, NS, pw.Ze, pw.Ae, pw.d0, pw.d1);
    poca_lin_t<0>(s, NS, H, H, dz0.f, prm + pn.oW[0], pw.dZp, nullptr);
    // the pool and the out-LayerNorm, W_out, the attention core
    hipLaunchKernelGGL(hk::poca_out_bwd_kernel, dim3(nblk(SR, 4)), dim3(256), 0, s, pw.dZp, pw.O, pw.ostat, SR, S, H, pw.dPre);
    ppo_wgrad(s, pw.part, H, H, SR, pw.dPre, H, pw.C, H, grad + pn.oWout, nullptr);
    ppo_colsum(s, pw.dPre, SR, H, H, grad + pn.obout);
    poca_lin_t<0>(s, SR, H, H, pw.dPre, prm + pn.oWout, pw.dC, nullptr);
    hipLaunchKernelGGL(hk::poca_attn_bwd_kernel, dim3(nblk(NS, 4)), dim3(256), 0, s, pw.Q, pw.K, pw.V, pw.alpha, pw.dC, NS, S, m, H, pw.dQs, pw.dKs, pw.dVs);
    hipLaunchKernelGGL(hk::poca_entsum_kernel, dim3(nblk((size_t)E2 * H)), dim3(256), 0, s, pw.dQs, pw.dKs, pw.dVs, pw.dPre, S, m, H, pw.dQ, pw.dK, pw.dV, pw.dR);
    // q, k, v: weights, biases, and the deltas into the normalised entities
    const struct { float* d; size_t oW, ob; float* dn; } qkv[3] = {{pw.dQ, pn.oWq, pn.obq, pw.dNq}, {pw.dK, pn.oWk, pn.obk, pw.dNk}, {pw.dV, pn.oWv, pn.obv, pw.dNv}};
    for (const auto& x : qkv) {
        ppo_wgrad(s, pw.part, H, H, E2, x.d, H, pw.N, H, grad + x.oW, nullptr);
        ppo_colsum(s, x.d, E2, H, H, grad + x.ob);
        poca_lin_t<0>(s, E2, H, H, x.d, prm + x.oW, x.dn, nullptr);
    }
    hipLaunchKernelGGL(hk::poca_ent_bwd_kernel, dim3(nblk(E2, 4)), dim3(256), 0, s, pw.dR, pw.dNq, pw.dNk, pw.dNv, pw.N, pw.estat, pw.Zent, E2, H, pw.dZent);
    // the two embeddings
    ppo_wgrad(s, pw.part, H, pn.in_dim, m, pw.dZent, H, w.X0, pn.in_dim, grad + pn.oWobs, nullptr);
    ppo_colsum(s, pw.dZent, m, H, H, grad + pn.obobs);
    float* dza = pw.dZent + (size_t)m * H;
    ppo_wgrad(s, pw.part, H, pn.n_act, m, dza, H, pw.XA, pn.n_act, grad + pn.oWact, nullptr);
    ppo_colsum(s, dza, m, H, H, grad + pn.obact);
    HK_HIP(h, hipGetLastError());
    t.last_m = m; t.last_mg = mg;
    return HK_OK;
}

// hk_ppo_advantages of a POCA trainer, between the frame's two halves: V and B over every group and V over the E bootstrap groups, in chunks; then
// the lambda-returns
int poca_values_and_returns(hk_handle h, hk_context::Ppo& t, const hk::PpoRows& P)
{
    const auto& ro = h->ro;
    const int S = P.S, G = P.R * P.E, n = G * S, nbt = P.E * S;
    int rc;
    const PpoRowBuf rows = ppo_rowbuf(h, t);
    const PocaRowBuf prows = poca_rowbuf(t);
    const int chunk = std::max(t.pcap, std::min(G + P.E, 4096));
    PpoWs w;
    PocaWs pw;
    if ((rc = ppo_ensure_ws(h, t, chunk * S, w))) return rc;
    if ((rc = poca_ensure_ws(h, t, chunk, pw))) return rc;
    hipStream_t s = h->stream;
    for (int base = 0; base < G + P.E; base += chunk) {
        const int mg = std::min(chunk, G + P.E - base);
        hipLaunchKernelGGL(hk::ppo_iota_kernel, dim3(nblk(mg)), dim3(256), 0, s, pw.gids, base, mg);
        poca_forward(s, t, P, w, pw, pw.gids, mg, 1);
        hipLaunchKernelGGL(hk::poca_scatter_kernel, dim3(nblk(mg * S)), dim3(256), 0, s, pw.out, pw.rid, mg * S, S, n, nbt, rows.v_old, prows.b_old, rows.v_boot,
                           nullptr, nullptr, nullptr);
    }
    hipLaunchKernelGGL(hk::poca_lambda_kernel, dim3(nblk(nbt)), dim3(256), 0, s, P, ro.at<float>(HK_RO_GROUP_REWARD), ro.at<float>(HK_RO_TERM_GROUP_REWARD),
                       rows.v_old, prows.b_old, rows.v_boot, t.cfg.gamma, t.cfg.lambd, prows.team, rows.adv, rows.ret);
    t.last_m = 0; t.last_mg = 0;          // the chunks went through the minibatch workspace (only here: see hk_ppo_advantages)
    return HK_OK;
}

// ... and of a PPO trainer: the critic over every row and the E S bootstrap rows, in chunks; then GAE
int ppo_values_and_gae(hk_handle h, hk_context::Ppo& t, const hk::PpoRows& P)
{
    const int n = t.n, nbt = P.E * P.S;
    const PpoRowBuf rows = ppo_rowbuf(h, t);
    PpoWs w;
    const int chunk = std::max(t.cap, std::min(n + nbt, 16384));
    int rc = ppo_ensure_ws(h, t, chunk, w);
    if (rc) return rc;
    hipStream_t s = h->stream;
    const hk::PpoNet& nc = t.critic;
    ppo_shadow_refresh(s, t);          // (only here: see hk_ppo_advantages)
    for (int base = 0; base < n + nbt; base += chunk) {
        const int m = std::min(chunk, n + nbt - base);
        hipLaunchKernelGGL(hk::ppo_iota_kernel, dim3(nblk(m)), dim3(256), 0, s, w.ids, base, m);
        ppo_gather(s, P, w.ids, m, 1, w.X0, w.valid);
        ppo_trunk_forward(s, t, nc, w.X0, m, w.Zc, w.Ac);
        hipLaunchKernelGGL(hk::ppo_value_kernel, dim3(nblk(m)), dim3(256), 0, s, w.Ac[nc.n_layers - 1].f, m, nc.hidden, t.param + nc.oWmu, t.param + nc.obmu,
                           w.ids, n, nbt, rows.v_old, rows.v_boot);
    }
    hipLaunchKernelGGL(hk::ppo_gae_kernel, dim3(nblk(nbt)), dim3(256), 0, s, P, rows.v_old, rows.v_boot, t.cfg.gamma, t.cfg.lambd, rows.adv, rows.ret);
    return HK_OK;
}

// ---- recurrent training (hk.h "PPO trainer" RECURRENT; device side in hk_ppo_lstm.h).  Everything below is reached only through a
// trainer made by hk_ppo_create_recurrent.

// a cell as the host sees it, the actor's (t.lnet) or a recurrent critic's (t.cnet): m wide on a trunk whose last layer is H wide, and the PARAMS
// offsets of W_ih [4m][H], W_hh [4m][m], b_ih and b_hh [4m].  Host only: the kernels take pointers and widths
struct PpoCell { int m, H; size_t oWih, oWhh, obih, obhh; };
template <typename Net> PpoCell ppo_cell(const Net& n) { return PpoCell{n.m, n.hidden, n.oWih, n.oWhh, n.obih, n.obhh}; }

// a cell's workspace at a capacity of M = L ms rows (sized by the minibatch, never by the rollout): the actor's (Ppo::rws), or a recurrent
// critic's (Ppo::cws) — the same pieces m_v wide, without the row ids and FIRST words, which are the actor workspace's for both
struct PpoLstmWs {
    int *rowids, *first;
    float *mem0, *bsum, *GZ, *hnew, *mbmem, *hprev, *cprev, *dH, *drec, *dcar, *part;
};

enum PpoCellOf { PPO_ACTOR_CELL, PPO_CRITIC_CELL };          // whose cell a workspace serves

size_t ppo_lstm_ws_layout(const hk_context::Ppo& t, PpoCellOf of, int M, PpoLstmWs* w)
{
    const bool critic = of == PPO_CRITIC_CELL;
    PpoBump a{w ? (char*)(critic ? t.cws : t.rws) : nullptr};
    auto fl = [&](size_t count) { return (float*)a.take(count * 4); };
    const PpoCell c = critic ? ppo_cell(t.cnet) : ppo_cell(t.lnet);
    const size_t Mz = (size_t)M, mc = (size_t)c.m;
    const size_t ms = (Mz + t.seq_len - 1) / t.seq_len;          // sequences at this capacity: M = L ms
    const int Ha = t.actor.hidden, Hc = t.critic.hidden, in = t.actor.in_dim, nb = t.actor.n_branch;
    // the largest weight gradient that goes through part: the cell's 4m x max(H, m) or a layer of the critic's trunk (a feed-forward critic's
    // goes through the actor's part) and, for the actor, the heads' or a layer of its own trunk; a sequence is at least one row, so ms <= M
    size_t mn = std::max(4 * mc * std::max((size_t)c.H, mc), (size_t)Hc * std::max(in, Hc));
    if (!critic) mn = std::max({mn, (size_t)(1 + nb) * mc, (size_t)Ha * std::max(in, Ha)});
    const size_t nz = (Mz + hk::PPO_KCH - 1) / hk::PPO_KCH;
    PpoLstmWs d{};
    if (!critic) { d.rowids = (int*)a.take(Mz * 4); d.first = (int*)a.take(Mz * 4); }
    d.mem0 = fl(ms * 2 * mc); d.bsum = fl(4 * mc);
    d.GZ = fl(Mz * 4 * mc); d.hnew = fl(Mz * mc); d.mbmem = fl(Mz * 2 * mc); d.hprev = fl(Mz * mc); d.cprev = fl(Mz * mc); d.dH = fl(Mz * mc);
    d.drec = fl(ms * mc); d.dcar = fl(ms * mc);
    d.part = fl(nz * mn);
    if (w) *w = d;
    return a.off;
}

// the two workspaces as they are allocated now
PpoLstmWs ppo_lstm_ws(const hk_context::Ppo& t) { PpoLstmWs w; ppo_lstm_ws_layout(t, PPO_ACTOR_CELL, t.rcap, &w); return w; }
PpoLstmWs ppo_lstm_cws(const hk_context::Ppo& t) { PpoLstmWs w; ppo_lstm_ws_layout(t, PPO_CRITIC_CELL, t.ccap, &w); return w; }

// the memories of a recurrent critic (Ppo::cmem): MEM_IN, MEM_OUT and the value pass's carry, [E S][2 m_v] each
struct PpoCriticMem { float *in, *out, *carry; size_t each; };
PpoCriticMem ppo_critic_mem(hk_handle h, const hk_context::Ppo& t)
{
    const size_t each = (size_t)h->cfg.num_envs * h->policy[t.policy].q.n_slots * 2 * t.critic_m;
    return PpoCriticMem{t.cmem, t.cmem + each, t.cmem + 2 * each, each};
}

// a cell's summed bias b_ih + b_hh [4m] ...
void ppo_cell_bsum(hipStream_t s, const hk_context::Ppo& t, const PpoCell& c, float* bsum)
{
    hipLaunchKernelGGL(hk::ppo_lstm_bsum_kernel, dim3(nblk(4 * c.m)), dim3(256), 0, s, t.param + c.obih, t.param + c.obhh, 4 * c.m, bsum);
}

// ... and its input projection over M rows of the trunk's last activations A: Zx [M][4m] = bsum + A W_ih^T (k ascending; fp32).  The two are
// apart because the value pass sums the bias once and projects every chunk
void ppo_cell_project(hipStream_t s, const hk_context::Ppo& t, const PpoCell& c, int M, PpoMat A, const float* bsum, float* Zx)
{
    ppo_product<0>(s, M, 4 * c.m, c.H, A, c.H, true, PpoMat(t.param + c.oWih), c.H, true, bsum, PpoMat(Zx), 4 * c.m, nullptr, c.H);
}

// a cell's forward over a minibatch's ms windows (M = L ms time-major rows) in its workspace r: the input projection over all rows at once, then
// the L steps from r.mem0
void ppo_cell_forward(hipStream_t s, const hk_context::Ppo& t, const PpoCell& c, const PpoLstmWs& r, PpoMat A, const int* first, int ms)
{
    const int L = t.seq_len;
    ppo_cell_bsum(s, t, c, r.bsum);
    ppo_cell_project(s, t, c, L * ms, A, r.bsum, r.GZ);
    const dim3 grid(nblk(c.m, hk::PPO_TN), nblk(ms, hk::PPO_TM));
    for (int tau = 0; tau < L; tau++)
        hipLaunchKernelGGL(hk::ppo_lstm_step_kernel, grid, dim3(256), 0, s, tau, ms, c.m, t.param + c.oWhh, r.mem0, first, r.GZ, r.hnew, r.mbmem, r.hprev, r.cprev);
}

// a cell's backward from r.dH = dL / dh' as the heads left it: the L steps in reverse, the cell's weight gradients over all rows at once (through
// r.part), the delta into the last layer of the trunk below (net, with its Z and A of the minibatch workspace), then that trunk
int ppo_cell_backward(hk_handle h, const hk_context::Ppo& t, const PpoCell& c, const PpoLstmWs& r, const hk::PpoNet& net, const PpoWs& w, float* const* Z,
                      const PpoMat* A, const int* first, int ms)
{
    hipStream_t s = h->stream;
    const int L = t.seq_len, M = L * ms, m = c.m, N = 4 * m, H = c.H, top = net.n_layers - 1;
    float* prm = t.param;
    float* grad = t.param + t.P;
    for (int tau = L - 1; tau >= 0; tau--) {
        hipLaunchKernelGGL(hk::ppo_lstm_back_kernel, dim3(nblk((size_t)ms * m)), dim3(256), 0, s, tau, ms, m, (int)(tau == L - 1), first, r.dH, r.drec, r.mbmem,
                           r.cprev, r.GZ, r.dcar);
        if (tau > 0)          // the recurrent delta to tau - 1: dG_tau [ms][4m] W_hh [4m][m]
            ppo_product<0>(s, ms, m, N, PpoMat(r.GZ + (size_t)tau * ms * N), N, true, PpoMat(prm + c.oWhh), m, false, nullptr, PpoMat(r.drec), m, nullptr, N);
    }
    ppo_wgrad(s, r.part, N, H, M, PpoMat(r.GZ), N, A[top], H, grad + c.oWih, nullptr);
    ppo_wgrad(s, r.part, N, m, M, PpoMat(r.GZ), N, PpoMat(r.hprev), m, grad + c.oWhh, nullptr);
    ppo_colsum(s, PpoMat(r.GZ), M, N, N, grad + c.obih);
    HK_HIP(h, hipMemcpyAsync(grad + c.obhh, grad + c.obih, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s));      // both biases: the same gradient
    ppo_product<2>(s, M, H, N, PpoMat(r.GZ), N, true, PpoMat(prm + c.oWih), H, false, nullptr, w.d0, H, Z[top], N);
    ppo_trunk_backward(s, t, net, r.part, w.X0, M, Z, A, w.d0, w.d1);
    return HK_OK;
}

// one recurrent minibatch: ms sequence ids -> M = L ms time-major rows; loss, stats, gradient into GRAD
int ppo_lstm_mb(hk_handle h, hk_context::Ppo& t, const int32_t* sids, int ms, float eps, float beta, bool acc)
{
    const int L = t.seq_len, mc = t.lnet.m;
    if ((long long)L * ms > 0x3FFFFFFF) return fail(h, HK_ERR_INVALID, "hk_ppo_minibatch: m x sequence_length rows do not fit");
    const int M = L * ms;
    PpoWs w;
    int rc = ppo_ensure_ws(h, t, M, w);
    if (rc) return rc;
    if (M > t.rcap && (rc = dev_grow(h, &t.rws, &t.rcap, M, ppo_lstm_ws_layout(t, PPO_ACTOR_CELL, M, nullptr)))) return rc;
    const PpoLstmWs r = ppo_lstm_ws(t);
    const int mv = t.critic_m;          // a recurrent critic (mv > 0): its cell's leg beside the actor's
    if (mv && M > t.ccap && (rc = dev_grow(h, &t.cws, &t.ccap, M, ppo_lstm_ws_layout(t, PPO_CRITIC_CELL, M, nullptr)))) return rc;
    const PpoLstmWs c = mv ? ppo_lstm_cws(t) : PpoLstmWs{};
    const PpoCell la = ppo_cell(t.lnet), lc = ppo_cell(t.cnet);
    hipStream_t s = h->stream;
    const hk::PpoRows P = ppo_rows(h, t);
    const auto& ro = h->ro;
    float* prm = t.param;
    float* grad = t.param + t.P;
    const hk::PpoNet& na = t.actor;
    const hk::PpoNet& nc = t.critic;
    const int La = na.n_layers - 1, Hc = nc.hidden, Lc = nc.n_layers - 1;
    // rows
    hipLaunchKernelGGL(hk::ppo_lstm_expand_kernel, dim3(nblk((size_t)M + (size_t)ms * 2 * mc)), dim3(256), 0, s, P, ro.at<float>(HK_RO_MEMORY), ro.mem_max, sids,
                       ms, L, t.n_seq, mc, r.rowids, r.first, r.mem0);
    ppo_gather(s, P, r.rowids, M, 0, w.X0, w.valid);
    hipLaunchKernelGGL(hk::ppo_count_kernel, dim3(1), dim3(256), 0, s, w.valid, M, w.n_valid);
    // forward: the trunks over all rows, then the actor's cell and, from CRITIC_MEMORY[k], a recurrent critic's
    ppo_trunk_forward(s, t, na, w.X0, M, w.Za, w.Aa);
    ppo_trunk_forward(s, t, nc, w.X0, M, w.Zc, w.Ac);
    ppo_cell_forward(s, t, la, r, w.Aa[La], r.first, ms);
    if (mv) {
        hipLaunchKernelGGL(hk::ppo_lstm_critic_mem0_kernel, dim3(nblk((size_t)ms * 2 * mv)), dim3(256), 0, s, t.cmemk, sids, ms, t.n_seq, mv, c.mem0);
        ppo_cell_forward(s, t, lc, c, w.Ac[Lc], r.first, ms);
    }
    // loss on h' (width m), per-row ids; a recurrent critic's value head reads its h' (nc.oWmu / obmu are the m_v-wide W_v / b_v)
    ppo_actor_loss(h, t, P, w, r.hnew, mc, PpoValueIn{mv ? c.hnew : w.Ac[Lc].f, mv ? mv : Hc, prm + nc.oWmu, prm + nc.obmu, r.rowids}, M, eps, beta, acc, sids, ms);
    // backward: the actor's heads (on h'), its cell and trunk
    ppo_head_grads(s, t, r.part, w, M, mc, PpoMat(r.hnew));
    hipLaunchKernelGGL(hk::ppo_lstm_head_back_kernel, dim3(nblk((size_t)M * mc)), dim3(256), 0, s, M, mc, 1 + na.n_branch, w.dhead, hk::PM_MAX_OUT, prm + na.oWmu,
                       prm + na.oWbr, r.dH);
    if ((rc = ppo_cell_backward(h, t, la, r, na, w, w.Za, w.Aa, r.first, ms))) return rc;
    if (mv) {
        // the recurrent critic: the value head's gradients and its delta onto h', then its cell and trunk
        ppo_wgrad(s, c.part, 1, mv, M, w.dv, 1, PpoMat(c.hnew), mv, grad + nc.oWmu, nullptr);
        ppo_colsum(s, w.dv, M, 1, 1, grad + nc.obmu);
        hipLaunchKernelGGL(hk::ppo_lstm_head_back_kernel, dim3(nblk((size_t)M * mv)), dim3(256), 0, s, M, mv, 1, w.dv, 1, prm + nc.oWmu, (const float*)nullptr, c.dH);
        if ((rc = ppo_cell_backward(h, t, lc, c, nc, w, w.Zc, w.Ac, r.first, ms))) return rc;
    } else {
        // critic (feed-forward on the stacked input, as a plain trainer's)
        ppo_value_head_back(s, t, r.part, M, Hc, w.dv, nc.oWmu, nc.obmu, w.Zc[Lc], w.Ac[Lc], w.d0);
        ppo_trunk_backward(s, t, nc, r.part, w.X0, M, w.Zc, w.Ac, w.d0, w.d1);
    }
    HK_HIP(h, hipGetLastError());
    t.last_m = M; t.last_ms = ms;
    return HK_OK;
}

// hk_ppo_advantages of a trainer with a recurrent critic (hk.h RECURRENT CRITIC): the critic run sequentially over the rows t = 0 .. R - 1 and the
// bootstrap step t = R of every (e, j), memory carried from MEM_IN; then GAE as a plain trainer's.  The R + 1 time steps go in chunks of T =
// value_chunk_steps, the E S sequences in tiles of sq, T sq rows of the order of the plain trainer's 16 384 at a time: gather, trunk and Zx over
// the chunk's rows at once (time-major), then ONE ppo_lstm_value_kernel launch for the chunk's T steps.  The bits depend on neither T nor sq:
// every row's chains are its own, and the carry between launches is exact.
int ppo_lstm_values_and_gae(hk_handle h, hk_context::Ppo& t, const hk::PpoRows& P)
{
    const auto& ro = h->ro;
    const int ES = P.E * P.S, mv = t.critic_m, N = 4 * mv, L = t.seq_len, K = (P.R + L - 1) / L;
    const PpoRowBuf rows = ppo_rowbuf(h, t);
    const PpoCriticMem cm = ppo_critic_mem(h, t);
    int rc;
    if ((rc = dev_grow(h, &t.cmemk, &t.cmemk_n, (size_t)K * cm.each, (size_t)K * cm.each * sizeof(float)))) return rc;
    t.cmem_k = K;
    // the tile of sequences follows from value_chunk_steps as given (16 384 rows / steps, whole 32-sequence blocks, at least one); the steps per
    // launch are at most the R + 1 there are
    const int Treq = t.value_chunk > 0 ? t.value_chunk : 16, T = std::min(Treq, P.R + 1);
    const int sq_cap = std::min(std::max(hk::PLV_TS, 16384 / Treq / hk::PLV_TS * hk::PLV_TS), ES);
    const size_t cap = (size_t)T * sq_cap;
    PpoWs w;
    if ((rc = ppo_ensure_ws(h, t, (int)cap, w))) return rc;
    if ((rc = dev_grow(h, &t.vws, &t.vcap, cap, (cap * N + N + cap) * sizeof(float)))) return rc;
    float* Zx = t.vws;
    float* bsum = t.vws + t.vcap * N;
    int* flags = (int*)(bsum + N);
    hipStream_t s = h->stream;
    const hk::PpoNet& nc = t.critic;
    const PpoCell lc = ppo_cell(t.cnet);
    const float* prm = t.param;
    if (t.cmem_gen != ro.gen) {          // a rollout this trainer has not seen: the memory its last value pass left is what this one starts from
        HK_HIP(h, hipMemcpyAsync(cm.in, cm.out, cm.each * sizeof(float), hipMemcpyDeviceToDevice, s));
        t.cmem_gen = ro.gen;
    }
    HK_HIP(h, hipMemcpyAsync(cm.carry, cm.in, cm.each * sizeof(float), hipMemcpyDeviceToDevice, s));
    ppo_cell_bsum(s, t, lc, bsum);
    const size_t lds = hk::ppo_lstm_value_lds_bytes(mv);
    for (int t0 = 0; t0 <= P.R; t0 += T) {
        const int Tc = std::min(T, P.R + 1 - t0);
        for (int p0 = 0; p0 < ES; p0 += sq_cap) {
            const int sq = std::min(sq_cap, ES - p0), m = Tc * sq;
            hipLaunchKernelGGL(hk::ppo_lstm_value_ids_kernel, dim3(nblk(m)), dim3(256), 0, s, P, w.ids, flags, t0, Tc, p0, sq);
            ppo_gather(s, P, w.ids, m, 1, w.X0, w.valid);
            ppo_trunk_forward(s, t, nc, w.X0, m, w.Zc, w.Ac);
            ppo_cell_project(s, t, lc, m, w.Ac[nc.n_layers - 1], bsum, Zx);
            hipLaunchKernelGGL(hk::ppo_lstm_value_kernel, dim3(nblk(sq, hk::PLV_TS)), dim3(64 * (mv / 32)), lds, s, P.R, ES, t0, Tc, p0, sq, mv, L, Zx, flags,
                               prm + lc.oWhh, prm + nc.oWmu, prm + nc.obmu, cm.carry, t.cmemk, cm.out, rows.v_old, rows.v_boot);
        }
    }
    hipLaunchKernelGGL(hk::ppo_gae_kernel, dim3(nblk(ES)), dim3(256), 0, s, P, rows.v_old, rows.v_boot, t.cfg.gamma, t.cfg.lambd, rows.adv, rows.ret);
    return HK_OK;
}

// one minibatch: loss, stats, gradient into GRAD (acc: the update's stats accumulator, or nullptr)
int ppo_mb(hk_handle h, hk_context::Ppo& t, const int32_t* ids, int m, float eps, float beta, bool acc)
{
    if (t.poca) return poca_mb(h, t, ids, m, eps, beta, acc);
    if (t.seq_len) return ppo_lstm_mb(h, t, ids, m, eps, beta, acc);
    PpoWs w;
    int rc = ppo_ensure_ws(h, t, m, w);
    if (rc) return rc;
    hipStream_t s = h->stream;
    const hk::PpoRows P = ppo_rows(h, t);
    const float* prm = t.param;
    const hk::PpoNet& nc = t.critic;
    const int Hc = nc.hidden, Lc = nc.n_layers - 1;      // Lc: the last trunk layer
    ppo_gather(s, P, ids, m, 0, w.X0, w.valid);
    hipLaunchKernelGGL(hk::ppo_count_kernel, dim3(1), dim3(256), 0, s, w.valid, m, w.n_valid);
    ppo_trunk_forward(s, t, t.actor, w.X0, m, w.Za, w.Aa);
    ppo_trunk_forward(s, t, nc, w.X0, m, w.Zc, w.Ac);
    ppo_actor_loss(h, t, P, w, w.Aa[t.actor.n_layers - 1].f, t.actor.hidden, PpoValueIn{w.Ac[Lc].f, Hc, prm + nc.oWmu, prm + nc.obmu, ids}, m, eps, beta, acc);
    ppo_actor_backward(s, t, w, m);
    // critic
    ppo_value_head_back(s, t, w.part, m, Hc, w.dv, nc.oWmu, nc.obmu, w.Zc[Lc], w.Ac[Lc], w.d0);
    ppo_trunk_backward(s, t, nc, w.part, w.X0, m, w.Zc, w.Ac, w.d0, w.d1);
    HK_HIP(h, hipGetLastError());
    t.last_m = m;
    return HK_OK;
}

// the HK_PPO_CLIP words and the partials of the norm, allocated (and zeroed) by the first clip-aware step
int ppo_ensure_clip(hk_handle h, hk_context::Ppo& t)
{
    if (t.clip) return HK_OK;
    const int parts = (int)((t.P + hk::PPO_GN_RUN - 1) / hk::PPO_GN_RUN);
    HK_HIP(h, hipMalloc(&t.clip, (size_t)(8 + parts) * sizeof(double)));
    t.clip_parts = parts;
    HK_HIP(h, hipMemsetAsync(t.clip, 0, (size_t)(8 + parts) * sizeof(double), h->stream));
    return HK_OK;
}

// one Adam step from GRAD; max_norm > 0: the clip-aware step of hk.h "LONG RUNS" (the norm's partials, then norm, coef and the step in one kernel)
int ppo_adam_step(hk_handle h, hk_context::Ppo& t, float lr, float max_norm = 0.0f)
{
    if (max_norm > 0.0f) { int rc = ppo_ensure_clip(h, t); if (rc) return rc; }
    t.adam_steps += 1;
    const float b1 = t.cfg.adam_beta1, b2 = t.cfg.adam_beta2;
    const float omb1 = (float)(1.0 - (double)b1), omb2 = (float)(1.0 - (double)b2);
    const float c1 = (float)(1.0 - std::pow((double)b1, t.adam_steps)), c2 = (float)(1.0 - std::pow((double)b2, t.adam_steps));
    float* p = t.param;
    if (max_norm > 0.0f) {
        double* part = t.clip + 8;
        hipLaunchKernelGGL(hk::ppo_gradnorm_partial_kernel, dim3(t.clip_parts), dim3(256), 0, h->stream, p + t.P, t.P, part);
        hipLaunchKernelGGL(hk::ppo_adam_clip_kernel, dim3(nblk(t.P)), dim3(256), 0, h->stream, p, p + t.P, p + 2 * t.P, p + 3 * t.P, t.P, b1, omb1, b2, omb2,
                           c1, c2, t.cfg.adam_eps, lr, part, t.clip_parts, max_norm, t.clip);
    } else {
        hipLaunchKernelGGL(hk::ppo_adam_kernel, dim3(nblk(t.P)), dim3(256), 0, h->stream, p, p + t.P, p + 2 * t.P, p + 3 * t.P, t.P, b1, omb1, b2, omb2, c1, c2,
                           t.cfg.adam_eps, lr);
    }
    ppo_shadow_refresh(h->stream, t);
    HK_HIP(h, hipGetLastError());
    return HK_OK;
}

// what changes or reads state that an open rollout owns
int ppo_refuse_open(hk_handle h, const char* fn)
{
    return h->ro.open ? fail(h, HK_ERR_INVALID, std::string(fn) + ": refused while a rollout is open (hk_rollout_close first)") : HK_OK;
}

int ppo_check(hk_handle h, int trainer, const char* fn, bool need_adv)
{
    if (trainer < 0 || trainer >= h->n_ppo) return fail(h, HK_ERR_INVALID, std::string(fn) + ": bad trainer index");
    const auto& t = h->ppo[trainer];
    if (!need_adv) return HK_OK;
    if (int rc = ppo_refuse_open(h, fn)) return rc;
    if (t.adv_gen != h->ro.gen) return fail(h, HK_ERR_INVALID, std::string(fn) + ": hk_ppo_advantages has not run on the current rollout");
    if (t.adv_stale) return fail(h, HK_ERR_INVALID, std::string(fn) + ": the actor's normaliser changed after hk_ppo_advantages (run it again)");
    return HK_OK;
}

// the preconditions of everything that reads the closed rollout's rows of a trainer (hk_ppo_advantages, hk_ppo_normalizer_update)
int ppo_check_rows(hk_handle h, const hk_context::Ppo& t, const char* fn)
{
    const auto& ro = h->ro;
    const std::string f(fn);
    if (int rc = ppo_refuse_open(h, fn)) return rc;
    if (ro.R == 0 || !ro.buf) return fail(h, HK_ERR_INVALID, f + ": no rollout yet (hk_rollout_begin ... hk_rollout_close)");
    if (ro.rows < 1) return fail(h, HK_ERR_INVALID, f + ": the rollout closed with no completed row");
    if (t.policy >= ro.npol) return fail(h, HK_ERR_INVALID, f + ": the rollout began before the trainer's actor was attached");
    return HK_OK;
}

// hk_ppo_normalizer_*: the trainer, and what every one of them refuses
int ppo_norm_check(hk_handle h, int trainer, const char* fn, bool need_state)
{
    int rc = ppo_check(h, trainer, fn, false);
    if (rc) return rc;
    const auto& t = h->ppo[trainer];
    const std::string f(fn);
    if (!h->policy[t.policy].q.normalize) return fail(h, HK_ERR_INVALID, f + ": the policy was attached with normalize == 0 (it has no statistics)");
    if ((rc = ppo_refuse_open(h, fn))) return rc;
    if (need_state && t.norm_steps < 1) return fail(h, HK_ERR_INVALID, f + ": no normaliser state (hk_ppo_normalizer_init or hk_ppo_normalizer_set first)");
    return HK_OK;
}

// a normaliser state as init / set accept it; what names the first offender
int ppo_norm_valid(hk_handle h, const char* fn, int64_t steps, const double* mean, const double* spread, int in_dim, const char* spread_name)
{
    const std::string f(fn);
    if (steps < 1) return fail(h, HK_ERR_INVALID, f + ": steps < 1");
    for (int k = 0; k < in_dim; k++) {
        if (!std::isfinite(mean[k])) return fail(h, HK_ERR_INVALID, f + ": mean[" + std::to_string(k) + "] is not finite");
        if (!(std::isfinite(spread[k]) && spread[k] > 0.0)) return fail(h, HK_ERR_INVALID, f + ": " + spread_name + "[" + std::to_string(k) + "] is not finite and > 0");
    }
    return HK_OK;
}

// the state's buffer, and the state (steps, m, M2) uploaded into it
int ppo_norm_store(hk_handle h, hk_context::Ppo& t, int64_t steps, const double* m, const double* m2)
{
    const hk::PolicyParams& q = h->policy[t.policy].q;
    const size_t K = (size_t)q.in_dim;
    if (!t.norm) HK_HIP(h, hipMalloc(&t.norm, (4 * K + q.stack) * sizeof(double)));
    HK_HIP(h, hipMemcpyAsync(t.norm, m, K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipMemcpyAsync(t.norm + K, m2, K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));          // (the host arrays are the caller's)
    t.norm_steps = steps;
    return HK_OK;
}

// the statistics of policy p changed: the advantages of its trainers are those of other inputs
void ppo_norm_stale(hk_handle h, int policy)
{
    for (int i = 0; i < h->n_ppo; i++) if (h->ppo[i].policy == policy) h->ppo[i].adv_stale = true;
}

// a recurrent actor's trunk as ppo_publish_kernel takes it: the net cut before the cell ln
hk::PpoNet ppo_trunk_only(hk::PpoNet net, const hk::PpoLstmNet& ln)
{
    net.count = ln.oWih;
    net.n_branch = 0;
    net.oWmu = net.obmu = net.ols = net.oWbr = net.obbr = net.count;      // (no element of the trunk matches a head)
    return net;
}

// the launches that move an actor between a flat copy (a trainer's PARAMS, a pool's slot) and a policy's inference copies (TO_POLICY: towards
// the policy): the whole net through ppo_publish_kernel or, of a recurrent actor (ln.m > 0), its trunk, then the cell and the m-wide heads
template <bool TO_POLICY>
void ppo_publish_actor(hipStream_t s, hk::PolicyDevice& pd, hk::PpoNet net, const hk::PpoLstmNet& ln, float* flat)
{
    if (ln.m) net = ppo_trunk_only(net, ln);
    hipLaunchKernelGGL(hk::ppo_publish_kernel<TO_POLICY>, dim3(nblk(net.count)), dim3(256), 0, s, pd.q, net, flat);
    if (ln.m) hipLaunchKernelGGL(hk::ppo_lstm_publish_kernel<TO_POLICY>, dim3(nblk(ln.end - ln.oWih)), dim3(256), 0, s, pd.q, pd.lq, pd.braw, ln, flat);
}

// hk_ppo_create and hk_ppo_create_poca (fn): the checks both start with, critic_checks() (the entry point's own refusals, in their place in the
// order), the config, the slot and the actor's layout; pack_critic(t, host) lays the critic out behind the actor and packs its parameters in
// that order; then PARAMS .. ADAM_V [4][P], zeroed, the critic uploaded and the actor's weights copied from the policy.  -> the trainer's index
// seq_len > 0: the call is hk_ppo_create_recurrent — the policy must HAVE memory, and the actor part carries the cell and the m-wide heads
template <typename Checks, typename Pack>
int ppo_create(hk_handle h, const char* fn, int policy, bool have_critic, const hk_ppo_config* cfg, Checks critic_checks, Pack pack_critic, int seq_len = 0)
{
    const std::string f = std::string(fn) + ": ";
    if (policy < 0 || policy >= h->n_policies) return fail(h, HK_ERR_INVALID, f + "bad policy index");
    if (h->n_ppo >= HK_MAX_POLICIES) return fail(h, HK_ERR_INVALID, f + "HK_MAX_POLICIES trainers already exist");
    if (!seq_len && h->policy[policy].lq.m > 0)
        return fail(h, HK_ERR_UNSUPPORTED, f + "policy: a recurrent actor (train it through hk_ppo_create_recurrent: hk.h \"PPO trainer\" RECURRENT)");
    if (seq_len && h->policy[policy].lq.m == 0) return fail(h, HK_ERR_INVALID, f + "policy: an actor without memory (train it through hk_ppo_create)");
    if (!have_critic) return fail(h, HK_ERR_INVALID, f + "NULL critic");
    const hk::PolicyParams& q = h->policy[policy].q;
    int rc = critic_checks(q);
    if (rc) return rc;
    hk_ppo_config d{0.99f, 0.95f, 1, 0.9f, 0.999f, 1e-8f, 0u};
    if (cfg) d = *cfg;
    if (!(d.adam_beta1 >= 0.0f && d.adam_beta1 < 1.0f && d.adam_beta2 >= 0.0f && d.adam_beta2 < 1.0f && d.adam_eps > 0.0f))
        return fail(h, HK_ERR_INVALID, f + "Adam constants out of range");
    auto& t = h->ppo[h->n_ppo];
    t = hk_context::Ppo{};
    t.policy = policy; t.cfg = d;
    t.actor.layout(q.in_dim, q.hidden, q.n_layers, q.n_branch, 0);
    if (seq_len) {
        // the trunk as laid out; the cell and the m-wide heads behind it (PpoLstmNet); the actor's head offsets follow
        hk::PpoLstmNet& ln = t.lnet;
        ln.layout(q.hidden, h->policy[policy].lq.m, q.n_branch, t.actor.oWmu);
        t.seq_len = seq_len;
        t.actor.oWmu = ln.oWmu; t.actor.obmu = ln.obmu; t.actor.ols = ln.ols; t.actor.oWbr = ln.oWbr; t.actor.obbr = ln.obbr;
        t.actor.count = ln.end;
    }
    std::vector<float> host;
    pack_critic(t, host);
    t.P = t.actor.count + host.size();
    hipError_t e = hipMalloc(&t.param, 4 * t.P * sizeof(float));
    if (e == hipSuccess) e = hipMemsetAsync(t.param, 0, 4 * t.P * sizeof(float), h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t.param + t.actor.count, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        ppo_publish_actor<false>(h->stream, h->policy[policy], t.actor, t.lnet, t.param);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {          // (the slot is not taken: free what was allocated)
        ppo_release(t);
        return fail(h, HK_ERR_HIP, f + hipGetErrorString(e));
    }
    return h->n_ppo++;
}

}  // namespace
}  // extern "C++"

static void ppo_release(hk_context::Ppo& t)
{
    (void)dev_free(t.param); (void)dev_free(t.rowbuf); (void)dev_free(t.ws); (void)dev_free(t.shadow); (void)dev_free(t.norm);
    (void)dev_free(t.norm_part); (void)dev_free(t.clip); (void)dev_free(t.prow); (void)dev_free(t.pws); (void)dev_free(t.rws);
    (void)dev_free(t.cws); (void)dev_free(t.cmem); (void)dev_free(t.cmemk); (void)dev_free(t.vws);
    t = hk_context::Ppo{};
}

extern "C++" {
namespace {
// what hk_ppo_create, hk_ppo_create_recurrent and hk_ppo_create_recurrent_critic refuse of the critic's trunk and value head (f: the entry
// point's name and ": ") ...
int ppo_critic_checks(hk_handle h, const std::string& f, const hk_policy_desc* c, const hk::PolicyParams& q)
{
    if (c->in_dim != q.in_dim) return fail(h, HK_ERR_INVALID, f + "the critic's in_dim differs from the actor's");
    if (c->hidden < 32 || c->hidden > HK_POLICY_MAX_HIDDEN || c->hidden % 32 || c->n_layers < 1 || c->n_layers > HK_POLICY_MAX_LAYERS || c->n_branch != 0)
        return fail(h, HK_ERR_INVALID, f + "critic hidden / n_layers out of the actor's limits, or n_branch != 0");
    for (int l = 0; l < c->n_layers; l++) if (!c->W[l] || !c->b[l]) return fail(h, HK_ERR_INVALID, f + "NULL critic layer weights");
    if (!c->W_mu || !c->b_mu) return fail(h, HK_ERR_INVALID, f + "NULL critic value head");
    return HK_OK;
}

// ... and the trunk's layers packed at t.critic's offsets into host, the critic's part of PARAMS (it starts at offset t.actor.count)
void ppo_pack_critic_trunk(const hk_context::Ppo& t, const hk_policy_desc* c, std::vector<float>& host)
{
    for (int l = 0; l < c->n_layers; l++) {
        const size_t nw = (size_t)c->hidden * (l == 0 ? c->in_dim : c->hidden);
        std::memcpy(&host[t.critic.oW[l] - t.actor.count], c->W[l], nw * 4);
        std::memcpy(&host[t.critic.ob[l] - t.actor.count], c->b[l], (size_t)c->hidden * 4);
    }
}

// hk_ppo_create and hk_ppo_create_recurrent: the feed-forward critic's checks and packing (fn names the entry point in the messages)
int ppo_create_ff(hk_handle h, const char* fn, int policy, const hk_policy_desc* c, const hk_ppo_config* cfg, int seq_len)
{
    const std::string f = std::string(fn) + ": ";
    auto checks = [&](const hk::PolicyParams& q) { return ppo_critic_checks(h, f, c, q); };
    auto pack = [&](hk_context::Ppo& t, std::vector<float>& host) {
        t.critic.layout(t.actor.in_dim, c->hidden, c->n_layers, 0, t.actor.count);
        host.resize(t.critic.count);
        ppo_pack_critic_trunk(t, c, host);
        std::memcpy(&host[t.critic.oWmu - t.actor.count], c->W_mu, (size_t)c->hidden * 4);
        host[t.critic.obmu - t.actor.count] = c->b_mu[0];
    };
    return ppo_create(h, fn, policy, c != nullptr, cfg, checks, pack, seq_len);
}
}  // namespace
}  // extern "C++"

int hk_ppo_create(hk_handle h, int policy, const hk_policy_desc* c, const hk_ppo_config* cfg)
{
    HK_NEED_ENV(h);
    return ppo_create_ff(h, "hk_ppo_create", policy, c, cfg, 0);
}

int hk_ppo_create_recurrent(hk_handle h, int policy, const hk_policy_desc* c, const hk_ppo_config* cfg, const hk_ppo_recurrent_desc* r)
{
    HK_NEED_ENV(h);
    if (!r) return fail(h, HK_ERR_INVALID, "hk_ppo_create_recurrent: NULL r (the hk_ppo_recurrent_desc)");
    if (r->sequence_length < 1) return fail(h, HK_ERR_INVALID, "hk_ppo_create_recurrent: sequence_length < 1");
    if (r->reserved != 0) return fail(h, HK_ERR_INVALID, "hk_ppo_create_recurrent: reserved != 0");
    return ppo_create_ff(h, "hk_ppo_create_recurrent", policy, c, cfg, r->sequence_length);
}

int hk_ppo_create_recurrent_critic(hk_handle h, int policy, const hk_policy_desc* c, const hk_policy_lstm_desc* cell, const hk_ppo_config* cfg,
                                   const hk_ppo_recurrent_critic_desc* r)
{
    HK_NEED_ENV(h);
    const std::string f = "hk_ppo_create_recurrent_critic: ";
    if (!r) return fail(h, HK_ERR_INVALID, f + "NULL r (the hk_ppo_recurrent_critic_desc)");
    if (!cell) return fail(h, HK_ERR_INVALID, f + "NULL critic_cell (the critic's hk_policy_lstm_desc)");
    if (r->sequence_length < 1) return fail(h, HK_ERR_INVALID, f + "sequence_length < 1");
    if (r->value_chunk_steps < 0) return fail(h, HK_ERR_INVALID, f + "value_chunk_steps < 0");
    if (r->reserved[0] != 0 || r->reserved[1] != 0) return fail(h, HK_ERR_INVALID, f + "reserved != 0");
    if (cell->reserved != 0) return fail(h, HK_ERR_INVALID, f + "critic_cell: reserved != 0");
    if (cell->memory_size & 1) return fail(h, HK_ERR_INVALID, f + "critic_cell: memory_size is odd (it holds h and c, m_v = memory_size / 2 each)");
    const int mv = cell->memory_size / 2;
    if (mv < 32 || mv > HK_POLICY_MAX_MEMORY / 2 || mv % 32)
        return fail(h, HK_ERR_INVALID, f + "critic_cell: memory_size: m_v = memory_size / 2 must be a multiple of 32 in [32, 128]");
    if (!cell->W_ih || !cell->W_hh || !cell->b_ih || !cell->b_hh) return fail(h, HK_ERR_INVALID, f + "critic_cell: NULL W_ih / W_hh / b_ih / b_hh");
    // the trunk's checks are the feed-forward critic's; the pack lays the cell and the m_v-wide value head behind the trunk
    auto checks = [&](const hk::PolicyParams& q) { return ppo_critic_checks(h, f, c, q); };
    auto pack = [&](hk_context::Ppo& t, std::vector<float>& host) {
        const size_t base = t.actor.count;
        const int Hc = c->hidden, N = 4 * mv;
        t.critic.layout(t.actor.in_dim, Hc, c->n_layers, 0, base);
        t.cnet.layout(Hc, mv, t.critic.oWmu);
        // from here on the value head is addressed through t.critic.oWmu / obmu alone (the loss, the value pass and the head's gradients read
        // them, as they do a feed-forward critic's); cnet.oWv / obv are read by this pack only
        t.critic.oWmu = t.cnet.oWv; t.critic.obmu = t.cnet.obv;
        t.critic.count = t.cnet.end - base;
        t.critic_m = mv; t.value_chunk = r->value_chunk_steps;
        host.resize(t.critic.count);
        auto put = [&](size_t off, const float* src, size_t k) { std::memcpy(&host[off - base], src, k * 4); };
        ppo_pack_critic_trunk(t, c, host);
        put(t.cnet.oWih, cell->W_ih, (size_t)N * Hc); put(t.cnet.oWhh, cell->W_hh, (size_t)N * mv);
        put(t.cnet.obih, cell->b_ih, N); put(t.cnet.obhh, cell->b_hh, N);
        put(t.cnet.oWv, c->W_mu, mv); put(t.cnet.obv, c->b_mu, 1);
    };
    const int idx = ppo_create(h, "hk_ppo_create_recurrent_critic", policy, c != nullptr, cfg, checks, pack, r->sequence_length);
    if (idx < 0) return idx;
    // MEM_IN, MEM_OUT and the carry, all zero; the value kernel's LDS (above 64 KB at m_v = 128)
    auto& t = h->ppo[idx];
    const size_t each = ppo_critic_mem(h, t).each;
    hipError_t e = hipMalloc(&t.cmem, 3 * each * sizeof(float));
    if (e == hipSuccess) e = hipMemsetAsync(t.cmem, 0, 3 * each * sizeof(float), h->stream);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)hk::ppo_lstm_value_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {          // (give the slot back)
        ppo_release(t);
        h->n_ppo--;
        return fail(h, HK_ERR_HIP, f + hipGetErrorString(e));
    }
    return idx;
}

int hk_ppo_advantages(hk_handle h, int trainer)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_advantages", false);
    if (rc) return rc;
    auto& t = h->ppo[trainer];
    const auto& ro = h->ro;
    if ((rc = ppo_check_rows(h, t, "hk_ppo_advantages"))) return rc;
    // The frame both trainers share: the rows' buffers and t.n, the trainer's own chunk loop and lambda / GAE kernel, then the normalisation and
    // the marks.  Two asymmetries inside the trainers' parts are intended.  ppo_shadow_refresh is issued on the PPO path only: a POCA trainer is
    // always fp32 and has no shadow.  last_m / last_mg are zeroed on the POCA path only, so the MB fields of a POCA trainer read "no minibatch
    // yet" after this call while a PPO trainer's keep what its last minibatch wrote (the PPO chunks write none of mb_mu / mb_logits / mb_v).
    const hk::PpoRows P = ppo_rows(h, t);
    const size_t n = (size_t)P.R * P.E * P.S, nbt = (size_t)P.E * P.S;
    if ((rc = dev_grow(h, &t.rowbuf, &t.rowbuf_n, 3 * n + nbt + n, (3 * n + nbt + n) * sizeof(float)))) return rc;
    if (t.poca && (rc = dev_grow(h, &t.prow, &t.prow_n, 2 * n, 2 * n * sizeof(float)))) return rc;
    t.n = (int)n;
    if (t.seq_len) {
        const long long nseq = (long long)((P.R + t.seq_len - 1) / t.seq_len) * P.E * P.S;
        t.n_seq = (int)nseq;          // (<= n)
    }
    if ((rc = t.poca ? poca_values_and_returns(h, t, P) : t.critic_m ? ppo_lstm_values_and_gae(h, t, P) : ppo_values_and_gae(h, t, P))) return rc;
    if (t.cfg.normalize_advantages) hipLaunchKernelGGL(hk::ppo_adv_norm_kernel, dim3(1), dim3(1024), 0, h->stream, ppo_rowbuf(h, t).adv, t.n);
    HK_HIP(h, hipGetLastError());
    t.adv_gen = ro.gen;
    t.perm_valid = false;
    t.adv_stale = false;
    return HK_OK;
}

int hk_ppo_minibatch(hk_handle h, int trainer, const int32_t* rows_dev, int m, float eps, float beta, float* stats)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_minibatch", true);
    if (rc) return rc;
    if (!rows_dev || m < 1) return fail(h, HK_ERR_INVALID, "hk_ppo_minibatch: NULL rows or m < 1");
    auto& t = h->ppo[trainer];
    ppo_shadow_refresh(h->stream, t);
    if ((rc = ppo_mb(h, t, rows_dev, m, eps, beta, false))) return rc;
    t.lb_from_update = false;
    if (stats) {
        HK_HIP(h, hipMemcpyAsync(stats, ppo_ws(t).stats, HK_PPO_STATS * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HK_HIP(h, hipStreamSynchronize(h->stream));
    }
    return HK_OK;
}

int hk_ppo_adam(hk_handle h, int trainer, float lr)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_adam", false);
    if (rc) return rc;
    return ppo_adam_step(h, h->ppo[trainer], lr);
}

int hk_ppo_publish(hk_handle h, int trainer)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_publish", false);
    if (rc) return rc;
    if ((rc = ppo_refuse_open(h, "hk_ppo_publish"))) return rc;
    auto& t = h->ppo[trainer];
    hk::PolicyDevice& pd = h->policy[t.policy];
    ppo_publish_actor<true>(h->stream, pd, t.actor, t.lnet, t.param);
    HK_HIP(h, hipGetLastError());
    // the bf16 inference copies, when a plain actor's policy has them: rebuilt from the fp32 copies just written (each an exact copy of its master,
    // so every weight is the master rounded once by ppo_bf16_rne: HK_PPO_SHADOW's element), whichever precision the policy is in now
    if (!t.seq_len && pd.wbf) HK_HIP(h, hk::policy_bf16_refresh(pd.q, pd.bq, h->stream));
    return HK_OK;
}

extern "C++" {
namespace {

// hk_ppo_update and hk_ppo_update_opt: epochs x (shuffle, minibatches, Adam), then publish.  max_norm 0 and target_kl 0 issue exactly the plain
// update's launches.  target_kl > 0: the stats accumulator is zeroed at the start of every epoch and read after it (one 64-byte copy and a
// synchronise per epoch); an epoch whose mean approx-KL exceeds target_kl is the last.  opt: the call is hk_ppo_update_opt.
int ppo_update_run(hk_handle h, int trainer, bool opt, int epochs, int minibatch, float lr, float eps, float beta, float max_norm,
                   float target_kl, float* stats, hk_ppo_update_report* report)
{
    auto& t = h->ppo[trainer];
    const int per = t.poca ? h->policy[t.policy].q.n_slots : 1;          // a POCA trainer's ids are groups of `per` agent rows
    const int n = t.seq_len ? t.n_seq : t.n / per;          // a recurrent trainer's ids are sequences of seq_len rows
    const int mb = std::min(minibatch, n), nmb = n / mb;
    const bool kl_stop = target_kl > 0.0f;
    int* perm = ppo_rowbuf(h, t).perm;
    PpoWs w;
    PocaWs pw{};
    int rc;
    if (t.seq_len && (long long)mb * t.seq_len > 0x3FFFFFFF) return fail(h, HK_ERR_INVALID, "hk_ppo_update: minibatch x sequence_length rows do not fit");
    if ((rc = ppo_ensure_ws(h, t, t.seq_len ? mb * t.seq_len : mb * per, w))) return rc;
    if (t.poca && (rc = poca_ensure_ws(h, t, mb, pw))) return rc;
    if (max_norm > 0.0f && (rc = ppo_ensure_clip(h, t))) return rc;
    if (opt && t.clip) HK_HIP(h, hipMemsetAsync(t.clip + 2, 0, 5 * sizeof(double), h->stream));       // the accumulating words [2 .. 6]
    ppo_shadow_refresh(h->stream, t);
    double acc[8] = {};
    bool have_acc = false;
    int run = 0, stopped = 0;
    for (int ep = 0; ep < epochs; ep++) {
        const bool last = ep == epochs - 1;
        if (last || kl_stop) HK_HIP(h, hipMemsetAsync(w.acc, 0, 8 * sizeof(double), h->stream));
        if (t.poca && (last || kl_stop)) HK_HIP(h, hipMemsetAsync(pw.pacc, 0, 2 * sizeof(double), h->stream));
        hipLaunchKernelGGL(hk::ppo_perm_kernel, dim3(nblk(n)), dim3(256), 0, h->stream, perm, n, t.cfg.seed, (uint32_t)t.epochs_done);
        t.epochs_done += 1;
        t.perm_valid = true;
        for (int b = 0; b < nmb; b++) {
            if ((rc = ppo_mb(h, t, perm + (size_t)b * mb, mb, eps, beta, last || kl_stop))) return rc;
            if ((rc = ppo_adam_step(h, t, lr, max_norm))) return rc;
        }
        run += 1;
        if (kl_stop) {
            HK_HIP(h, hipMemcpyAsync(acc, w.acc, sizeof(acc), hipMemcpyDeviceToHost, h->stream));
            HK_HIP(h, hipStreamSynchronize(h->stream));
            have_acc = true;
            if (!last && acc[3] / (acc[6] > 0 ? acc[6] : 1.0) > (double)target_kl) { stopped = 1; break; }
        }
    }
    if ((rc = hk_ppo_publish(h, trainer))) return rc;
    t.lb_from_update = true;
    if (stats || report) {
        double words[8] = {};
        if (!have_acc) HK_HIP(h, hipMemcpyAsync(acc, w.acc, sizeof(acc), hipMemcpyDeviceToHost, h->stream));
        if (report && max_norm > 0.0f) HK_HIP(h, hipMemcpyAsync(words, t.clip, sizeof(words), hipMemcpyDeviceToHost, h->stream));
        HK_HIP(h, hipStreamSynchronize(h->stream));
        const double d = acc[6] > 0 ? acc[6] : 1.0;
        if (stats) for (int q = 0; q < HK_PPO_STATS; q++) stats[q] = (float)(acc[q] / d);
        if (report) {
            hk_ppo_update_report r{};
            r.epochs_run = run; r.minibatches_run = run * nmb; r.stopped_by_kl = stopped;
            r.clipped_steps = (int32_t)words[3]; r.nonfinite_steps = (int32_t)words[4];
            r.last_epoch_kl = acc[3] / d;
            const double fin = words[2] - words[4];
            r.grad_norm_mean = fin > 0 ? words[5] / fin : 0.0;
            r.grad_norm_max = words[6];
            *report = r;
        }
    }
    return HK_OK;
}

// max_grad_norm / target_kl as hk_ppo_update_opts states them: 0 off, > 0 on (+inf allowed for the norm), < 0 or NaN refused
int ppo_opt_range(hk_handle h, const char* fn, const char* name, float v, bool inf_ok)
{
    if (v >= 0.0f && (inf_ok || std::isfinite(v))) return HK_OK;
    return fail(h, HK_ERR_INVALID, std::string(fn) + ": " + name + " is negative, NaN" + (inf_ok ? "" : " or infinite") + " (0: off)");
}

}  // namespace
}  // extern "C++"

int hk_ppo_update(hk_handle h, int trainer, int epochs, int minibatch, float lr, float eps, float beta, float* stats)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_update", true);
    if (rc) return rc;
    if (epochs < 1 || minibatch < 1) return fail(h, HK_ERR_INVALID, "hk_ppo_update: epochs < 1 or minibatch < 1");
    return ppo_update_run(h, trainer, false, epochs, minibatch, lr, eps, beta, 0.0f, 0.0f, stats, nullptr);
}

int hk_ppo_update_opt(hk_handle h, int trainer, const hk_ppo_update_opts* o, float* stats, hk_ppo_update_report* report)
{
    HK_NEED_ENV(h);
    const char* fn = "hk_ppo_update_opt";
    int rc = ppo_check(h, trainer, fn, true);
    if (rc) return rc;
    if (!o) return fail(h, HK_ERR_INVALID, "hk_ppo_update_opt: NULL opts");
    if (o->epochs < 1) return fail(h, HK_ERR_INVALID, "hk_ppo_update_opt: epochs < 1");
    if (o->minibatch < 1) return fail(h, HK_ERR_INVALID, "hk_ppo_update_opt: minibatch < 1");
    if ((rc = ppo_opt_range(h, fn, "max_grad_norm", o->max_grad_norm, true))) return rc;
    if ((rc = ppo_opt_range(h, fn, "target_kl", o->target_kl, false))) return rc;
    if (o->reserved != 0) return fail(h, HK_ERR_INVALID, "hk_ppo_update_opt: reserved != 0");
    return ppo_update_run(h, trainer, true, o->epochs, o->minibatch, o->lr, o->eps, o->beta, o->max_grad_norm, o->target_kl, stats, report);
}

int hk_ppo_adam_clipped(hk_handle h, int trainer, float lr, float max_grad_norm)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_adam_clipped", false);
    if (rc) return rc;
    if (!(max_grad_norm > 0.0f)) return fail(h, HK_ERR_INVALID, "hk_ppo_adam_clipped: max_grad_norm is not > 0 (NaN included; +inf measures only)");
    return ppo_adam_step(h, h->ppo[trainer], lr, max_grad_norm);
}

int hk_ppo_get_counters(hk_handle h, int trainer, int64_t* adam_steps, int64_t* epochs_done)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_get_counters", false);
    if (rc) return rc;
    const auto& t = h->ppo[trainer];
    if (adam_steps) *adam_steps = t.adam_steps;
    if (epochs_done) *epochs_done = t.epochs_done;
    return HK_OK;
}

int hk_ppo_set_counters(hk_handle h, int trainer, int64_t adam_steps, int64_t epochs_done)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_set_counters", false);
    if (rc) return rc;
    if ((rc = ppo_refuse_open(h, "hk_ppo_set_counters"))) return rc;
    if (adam_steps < 0 || adam_steps > INT32_MAX) return fail(h, HK_ERR_INVALID, "hk_ppo_set_counters: adam_steps outside [0, INT32_MAX]");
    if (epochs_done < 0 || epochs_done > INT32_MAX) return fail(h, HK_ERR_INVALID, "hk_ppo_set_counters: epochs_done outside [0, INT32_MAX]");
    auto& t = h->ppo[trainer];
    t.adam_steps = (int)adam_steps; t.epochs_done = (int)epochs_done;
    return HK_OK;
}

int hk_ppo_normalizer_init(hk_handle h, int trainer, int64_t steps)
{
    HK_NEED_ENV(h);
    int rc = ppo_norm_check(h, trainer, "hk_ppo_normalizer_init", false);
    if (rc) return rc;
    auto& t = h->ppo[trainer];
    const hk::PolicyParams& q = h->policy[t.policy].q;
    const int K = q.in_dim;
    std::vector<float> mean(K), sdev(K);
    HK_HIP(h, hipMemcpyAsync(mean.data(), q.mean, K * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipMemcpyAsync(sdev.data(), q.std, K * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    std::vector<double> m(mean.begin(), mean.end()), sd(sdev.begin(), sdev.end()), m2(K);
    if ((rc = ppo_norm_valid(h, "hk_ppo_normalizer_init", steps, m.data(), sd.data(), K, "std"))) return rc;
    for (int k = 0; k < K; k++) m2[k] = sd[k] * sd[k] * (double)steps;
    return ppo_norm_store(h, t, steps, m.data(), m2.data());          // (the published values stay as they are)
}

int hk_ppo_normalizer_set(hk_handle h, int trainer, int64_t steps, const double* mean, const double* m2)
{
    HK_NEED_ENV(h);
    int rc = ppo_norm_check(h, trainer, "hk_ppo_normalizer_set", false);
    if (rc) return rc;
    if (!mean || !m2) return fail(h, HK_ERR_INVALID, "hk_ppo_normalizer_set: NULL mean or m2");
    auto& t = h->ppo[trainer];
    const hk::PolicyParams& q = h->policy[t.policy].q;
    if ((rc = ppo_norm_valid(h, "hk_ppo_normalizer_set", steps, mean, m2, q.in_dim, "m2"))) return rc;
    if ((rc = ppo_norm_store(h, t, steps, mean, m2))) return rc;
    hipLaunchKernelGGL(hk::ppo_norm_publish_kernel, dim3(nblk(q.in_dim)), dim3(256), 0, h->stream, t.norm, const_cast<float*>(q.mean), const_cast<float*>(q.std),
                       q.in_dim, (double)steps);
    HK_HIP(h, hipGetLastError());
    ppo_norm_stale(h, t.policy);
    return HK_OK;
}

int hk_ppo_normalizer_get(hk_handle h, int trainer, int64_t* steps, double* mean, double* m2)
{
    HK_NEED_ENV(h);
    int rc = ppo_norm_check(h, trainer, "hk_ppo_normalizer_get", true);
    if (rc) return rc;
    const auto& t = h->ppo[trainer];
    const size_t K = (size_t)h->policy[t.policy].q.in_dim;
    if (mean) HK_HIP(h, hipMemcpyAsync(mean, t.norm, K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (m2) HK_HIP(h, hipMemcpyAsync(m2, t.norm + K, K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    if (steps) *steps = t.norm_steps;
    return HK_OK;
}

int hk_ppo_normalizer_update(hk_handle h, int trainer)
{
    HK_NEED_ENV(h);
    int rc = ppo_norm_check(h, trainer, "hk_ppo_normalizer_update", true);
    if (rc) return rc;
    auto& t = h->ppo[trainer];
    if ((rc = ppo_check_rows(h, t, "hk_ppo_normalizer_update"))) return rc;
    const hk::PpoRows P = ppo_rows(h, t);
    const hk::PolicyParams& q = h->policy[t.policy].q;
    const int K = P.in_dim, W = 2 * K + P.stack;
    const long long n = (long long)P.R * P.E * P.S;
    // the fixed partition: the items (u, e, j) in order, cut into at most PPO_NORM_MAXWG runs of whole trips
    const int DL = std::min(P.D, 256), trip = (256 / DL) * hk::PPO_NORM_U;
    const long long items = (long long)(P.R + P.stack - 1) * P.E * P.S;
    long long ipw = (items + hk::PPO_NORM_MAXWG - 1) / hk::PPO_NORM_MAXWG;
    ipw = (ipw + trip - 1) / trip * trip;
    if (items + ipw > 0x7FFFFFFFLL) return fail(h, HK_ERR_UNSUPPORTED, "hk_ppo_normalizer_update: more than 2^31 recorded observations");
    const int nwg = (int)((items + ipw - 1) / ipw);
    if ((rc = dev_grow(h, &t.norm_part, &t.norm_part_wg, nwg, (size_t)nwg * W * sizeof(double)))) return rc;
    hipStream_t s = h->stream;
    double* sums = t.norm + 2 * (size_t)K;
    const dim3 grid(nwg, (P.stack + hk::PPO_NORM_Q - 1) / hk::PPO_NORM_Q, (P.D + 255) / 256);
    hipLaunchKernelGGL(hk::ppo_norm_partial_kernel, grid, dim3(256), 0, s, P, t.norm, (int)ipw, t.norm_part);
    hipLaunchKernelGGL(hk::ppo_norm_combine_kernel, dim3(nblk(W, 256 / hk::PPO_NORM_SEG)), dim3(256), 0, s, t.norm_part, nwg, W, sums);
    const int64_t N1 = t.norm_steps + n;
    hipLaunchKernelGGL(hk::ppo_norm_finalise_kernel, dim3(nblk(K)), dim3(256), 0, s, sums, t.norm, const_cast<float*>(q.mean), const_cast<float*>(q.std), K,
                       P.D, (double)n, (double)N1);
    HK_HIP(h, hipGetLastError());
    t.norm_steps = N1;
    ppo_norm_stale(h, t.policy);
    return HK_OK;
}

int hk_ppo_set_precision(hk_handle h, int trainer, int precision)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_set_precision", false);
    if (rc) return rc;
    if (precision != HK_PPO_PREC_F32 && precision != HK_PPO_PREC_BF16) return fail(h, HK_ERR_INVALID, "hk_ppo_set_precision: unknown precision");
    auto& t = h->ppo[trainer];
    if (t.poca && precision != HK_PPO_PREC_F32) return fail(h, HK_ERR_UNSUPPORTED, "hk_ppo_set_precision: a POCA trainer has no bf16 products (hk.h \"POCA\")");
    if (t.seq_len && precision != HK_PPO_PREC_F32)
        return fail(h, HK_ERR_UNSUPPORTED, "hk_ppo_set_precision: precision: a recurrent trainer has no bf16 products (hk.h \"PPO trainer\" RECURRENT)");
    if (precision == t.prec) return HK_OK;
    // the workspace is laid out per precision: drop it once the stream is done with it (the next minibatch allocates the other layout)
    HK_HIP(h, hipStreamSynchronize(h->stream));
    t.cap = 0; t.last_m = 0;
    HK_HIP(h, dev_free(t.ws));
    if (precision == HK_PPO_PREC_BF16 && !t.shadow) {
        t.shadow_pad = (8 - t.actor.count % 8) % 8;
        HK_HIP(h, hipMalloc(&t.shadow, (t.P + t.shadow_pad) * sizeof(uint16_t)));
        HK_HIP(h, hipMemsetAsync(t.shadow, 0, (t.P + t.shadow_pad) * sizeof(uint16_t), h->stream));
    }
    t.prec = precision;          // (before the refresh, which looks at it)
    ppo_shadow_refresh(h->stream, t);
    HK_HIP(h, hipGetLastError());
    return HK_OK;
}

int hk_ppo_get_precision(hk_handle h, int trainer)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "NULL handle");
    if (trainer < 0 || trainer >= h->n_ppo) return fail(h, HK_ERR_INVALID, "hk_ppo_get_precision: bad trainer index");
    return h->ppo[trainer].prec;
}

int hk_ppo_gemm_bf16(hk_handle h, int epi, int M, int N, int K, const void* A_dev, const void* B_dev, const float* bias_dev, const float* aux_dev, float* C_dev)
{
    HK_NEED_ENV(h);
    if (epi < 0 || epi > 2) return fail(h, HK_ERR_INVALID, "hk_ppo_gemm_bf16: unknown epi");
    if (M < 1 || N < 1 || K < 1) return fail(h, HK_ERR_INVALID, "hk_ppo_gemm_bf16: M, N, K must be positive");
    if (!A_dev || !B_dev || !C_dev || (epi == 2 && !aux_dev)) return fail(h, HK_ERR_INVALID, "hk_ppo_gemm_bf16: NULL operand");
    const PpoMat A((uint16_t*)A_dev), B((uint16_t*)B_dev);          // (read only)
    hipStream_t s = h->stream;
    if (epi == 0) {
        float* part = nullptr;
        const size_t nz = ((size_t)K + hk::PPO_KCH - 1) / hk::PPO_KCH;
        HK_HIP(h, hipMalloc(&part, nz * M * N * sizeof(float)));
        ppo_wgrad(s, part, M, N, K, A, M, B, N, C_dev, nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        (void)hipFree(part);
        HK_HIP(h, e);
        return HK_OK;
    }
    if (epi == 1) ppo_product<1>(s, M, N, K, A, K, true, B, K, true, bias_dev, C_dev, N, nullptr, K);
    else ppo_product<2>(s, M, N, K, A, K, true, B, N, false, nullptr, C_dev, N, const_cast<float*>(aux_dev), K);
    HK_HIP(h, hipGetLastError());
    return HK_OK;
}

void* hk_ppo_ptr(hk_handle h, int trainer, int field)
{
    if (!h) { fail(nullptr, HK_ERR_INVALID, "NULL handle"); return nullptr; }
    if (trainer < 0 || trainer >= h->n_ppo) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: bad trainer index"); return nullptr; }
    const auto& t = h->ppo[trainer];
    const bool critic_field = field >= HK_PPO_CRITIC_MEMORY && field <= HK_PPO_MB_CRITIC_MEMORY;
    if ((field < 0 || field >= HK_PPO_FIELDS) && field != HK_PPO_MB_MEMORY && !critic_field) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: bad field"); return nullptr; }
    if (critic_field) {          // (RECURRENT CRITIC)
        if (!t.critic_m) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: the HK_PPO_CRITIC_* fields belong to a trainer with a recurrent critic"); return nullptr; }
        if (field == HK_PPO_CRITIC_MEM_IN) return ppo_critic_mem(h, t).in;
        if (field == HK_PPO_CRITIC_MEM_OUT) return ppo_critic_mem(h, t).out;
        if (field == HK_PPO_CRITIC_MEMORY) {
            if (t.adv_gen < 0) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: hk_ppo_advantages has not run"); return nullptr; }
            return t.cmemk;
        }
        if (t.last_m == 0) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: no minibatch yet"); return nullptr; }
        return ppo_lstm_cws(t).mbmem;
    }
    if (field <= HK_PPO_ADAM_V) return t.param + (size_t)field * t.P;
    if (field <= HK_PPO_RET) {
        if (t.adv_gen < 0) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: hk_ppo_advantages has not run"); return nullptr; }
        const PpoRowBuf rows = ppo_rowbuf(h, t);
        return field == HK_PPO_V_OLD ? rows.v_old : field == HK_PPO_ADV ? rows.adv : rows.ret;
    }
    if (field == HK_PPO_PERM) {
        if (!t.perm_valid) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: no hk_ppo_update on the current advantages"); return nullptr; }
        return ppo_rowbuf(h, t).perm;
    }
    if (field == HK_PPO_NORM_MEAN || field == HK_PPO_NORM_STD) {
        const hk::PolicyParams& q = h->policy[t.policy].q;
        if (!q.normalize) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: the policy was attached with normalize == 0"); return nullptr; }
        return const_cast<float*>(field == HK_PPO_NORM_MEAN ? q.mean : q.std);
    }
    if (field == HK_PPO_SHADOW) {
        if (!t.shadow) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: the trainer has never been in HK_PPO_PREC_BF16"); return nullptr; }
        return t.shadow;
    }
    if (field == HK_PPO_CLIP) {
        if (!t.clip) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: no clip-aware step yet"); return nullptr; }
        return t.clip;
    }
    if (field == HK_PPO_MB_MEMORY && !t.seq_len) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: HK_PPO_MB_MEMORY belongs to a recurrent trainer"); return nullptr; }
    if (t.last_m == 0) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: no minibatch yet"); return nullptr; }
    if (field == HK_PPO_MB_MEMORY) return ppo_lstm_ws(t).mbmem;
    if (t.poca && field == HK_PPO_MB_VALUE) {          // one value per group
        return poca_ws(h, t).mb_v;
    }
    const PpoWs w = ppo_ws(t);
    return field == HK_PPO_MB_MU ? (void*)w.mb_mu : field == HK_PPO_MB_LOGITS ? (void*)w.mb_logits : (void*)w.mb_v;
}

int hk_ppo_count(hk_handle h, int trainer, int field)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "NULL handle");
    if (trainer < 0 || trainer >= h->n_ppo) return fail(h, HK_ERR_INVALID, "hk_ppo_count: bad trainer index");
    const auto& t = h->ppo[trainer];
    if (field >= HK_PPO_CRITIC_MEMORY && field <= HK_PPO_MB_CRITIC_MEMORY) {          // (RECURRENT CRITIC; 0 on every other trainer)
        if (!t.critic_m) return 0;
        const size_t each = ppo_critic_mem(h, t).each;
        if (field == HK_PPO_CRITIC_MEMORY) return t.adv_gen < 0 ? 0 : (int)(t.cmem_k * each);
        return field == HK_PPO_MB_CRITIC_MEMORY ? t.last_m * 2 * t.critic_m : (int)each;
    }
    if ((field < 0 || field >= HK_PPO_FIELDS) && field != HK_PPO_MB_MEMORY) return fail(h, HK_ERR_INVALID, "hk_ppo_count: bad field");
    if (field <= HK_PPO_ADAM_V) return (int)t.P;
    if (field <= HK_PPO_RET) return t.adv_gen < 0 ? 0 : t.n;
    if (field == HK_PPO_PERM) return t.perm_valid ? (t.seq_len ? t.n_seq : t.poca ? t.n / h->policy[t.policy].q.n_slots : t.n) : 0;
    if (field == HK_PPO_MB_MEMORY) return t.seq_len ? t.last_m * 2 * t.lnet.m : 0;
    if (field == HK_PPO_SHADOW) return t.shadow ? (int)(t.P + t.shadow_pad) : 0;
    if (field == HK_PPO_CLIP) return t.clip ? 8 : 0;
    if (field == HK_PPO_NORM_MEAN || field == HK_PPO_NORM_STD) return h->policy[t.policy].q.normalize ? h->policy[t.policy].q.in_dim : 0;
    if (t.poca && field == HK_PPO_MB_VALUE) return t.last_mg;
    return field == HK_PPO_MB_LOGITS ? t.last_m * t.actor.n_branch : t.last_m;
}

int hk_ppo_create_poca(hk_handle h, int policy, const hk_poca_critic_desc* c, const hk_ppo_config* cfg)
{
    HK_NEED_ENV(h);
    auto bad = [&](const char* what) { return fail(h, HK_ERR_INVALID, std::string("hk_ppo_create_poca: ") + what); };
    auto checks = [&](const hk::PolicyParams& q) {
        if (!h->cfg.rewards) return bad("hk_config.rewards == 0 (the rows carry no rewards)");
        const int S = q.n_slots;
        if (S < 2 || S > HK_POCA_MAX_GROUP) return bad("the policy's slots are not a group of 2 .. HK_POCA_MAX_GROUP agents");
        const int team = h->cfg.team_of[q.slots[0]];
        int members = 0;
        for (int a = 0; a < h->cfg.num_agents; a++) members += h->cfg.team_of[a] == team;
        for (int j = 0; j < S; j++) if (h->cfg.team_of[q.slots[j]] != team) return bad("the policy's slots are not on one team");
        if (members != S) return bad("the policy's slots are not every member of their team");
        if (c->hidden < 4 || c->hidden > HK_POLICY_MAX_HIDDEN || c->hidden % 4) return bad("hidden is not a multiple of 4 in [4, HK_POLICY_MAX_HIDDEN]");
        if (c->n_layers < 1 || c->n_layers > HK_POLICY_MAX_LAYERS) return bad("n_layers outside [1, HK_POLICY_MAX_LAYERS]");
        if (c->reserved0 != 0 || c->reserved1 != 0) return bad("reserved != 0");
        if (!c->W_obs || !c->b_obs || !c->W_act || !c->b_act || !c->W_q || !c->b_q || !c->W_k || !c->b_k || !c->W_v || !c->b_v || !c->W_out || !c->b_out ||
            !c->w_val || !c->b_val)
            return bad("a NULL array");
        for (int l = 0; l < c->n_layers; l++) if (!c->W[l] || !c->b[l]) return bad("a NULL array (encoder)");
        return (int)HK_OK;
    };
    auto pack = [&](hk_context::Ppo& t, std::vector<float>& host) {
        t.poca = true;
        t.pnet.layout(t.actor.in_dim, t.actor.n_branch, c->hidden, c->n_layers, t.actor.count);
        const hk::PocaNet& pn = t.pnet;
        const size_t H = (size_t)c->hidden, base = t.actor.count;
        host.resize(pn.count);
        auto put = [&](size_t off, const float* src, size_t k) { std::memcpy(&host[off - base], src, k * 4); };
        put(pn.oWobs, c->W_obs, H * pn.in_dim); put(pn.obobs, c->b_obs, H);
        put(pn.oWact, c->W_act, H * pn.n_act); put(pn.obact, c->b_act, H);
        put(pn.oWq, c->W_q, H * H); put(pn.obq, c->b_q, H); put(pn.oWk, c->W_k, H * H); put(pn.obk, c->b_k, H);
        put(pn.oWv, c->W_v, H * H); put(pn.obv, c->b_v, H); put(pn.oWout, c->W_out, H * H); put(pn.obout, c->b_out, H);
        for (int l = 0; l < c->n_layers; l++) { put(pn.oW[l], c->W[l], H * H); put(pn.ob[l], c->b[l], H); }
        put(pn.owval, c->w_val, H); put(pn.obval, c->b_val, 1);
    };
    return ppo_create(h, "hk_ppo_create_poca", policy, c != nullptr, cfg, checks, pack);
}

extern "C++" {
namespace {
// a POCA trainer and field -> 0, or a failure naming fn
int poca_field_check(hk_handle h, int trainer, int field, const char* fn)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "NULL handle");
    if (trainer < 0 || trainer >= h->n_ppo) return fail(h, HK_ERR_INVALID, std::string(fn) + ": bad trainer index");
    if (!h->ppo[trainer].poca) return fail(h, HK_ERR_INVALID, std::string(fn) + ": not a POCA trainer (hk_ppo_create_poca)");
    if (field < 0 || field >= HK_POCA_FIELDS) return fail(h, HK_ERR_INVALID, std::string(fn) + ": bad field");
    return HK_OK;
}
}  // namespace
}  // extern "C++"

void* hk_poca_ptr(hk_handle h, int trainer, int field)
{
    if (poca_field_check(h, trainer, field, "hk_poca_ptr")) return nullptr;
    const auto& t = h->ppo[trainer];
    if (field == HK_POCA_MB_BASELINE) {
        if (t.last_mg == 0) { fail(h, HK_ERR_INVALID, "hk_poca_ptr: no minibatch yet"); return nullptr; }
        return poca_ws(h, t).brow;
    }
    if (t.adv_gen < 0) { fail(h, HK_ERR_INVALID, "hk_poca_ptr: hk_ppo_advantages has not run"); return nullptr; }
    const PocaRowBuf r = poca_rowbuf(t);
    return field == HK_POCA_B_OLD ? r.b_old : r.team;
}

int hk_poca_count(hk_handle h, int trainer, int field)
{
    int rc = poca_field_check(h, trainer, field, "hk_poca_count");
    if (rc) return rc;
    const auto& t = h->ppo[trainer];
    if (field == HK_POCA_MB_BASELINE) return t.last_m;
    return t.adv_gen < 0 ? 0 : t.n;
}

int hk_poca_stats(hk_handle h, int trainer, float* out)
{
    int rc = poca_field_check(h, trainer, 0, "hk_poca_stats");
    if (rc) return rc;
    if (!out) return fail(h, HK_ERR_INVALID, "hk_poca_stats: NULL out");
    const auto& t = h->ppo[trainer];
    if (!t.pws || (t.last_mg == 0 && !t.lb_from_update)) return fail(h, HK_ERR_INVALID, "hk_poca_stats: no minibatch or update yet");
    const PocaWs pw = poca_ws(h, t);
    float st[HK_POCA_STATS] = {};
    double acc[2] = {};
    HK_HIP(h, hipMemcpyAsync(st, pw.pstats, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipMemcpyAsync(acc, pw.pacc, sizeof(acc), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    out[0] = t.lb_from_update ? (float)(acc[0] / (acc[1] > 0 ? acc[1] : 1.0)) : st[0];
    out[1] = 0.0f;
    return HK_OK;
}

// ------------------------------------------------------------------ self-play (hk.h "SELF-PLAY"; device side of the statistics in hk_selfplay.h)
extern "C++" {
namespace {

// pool / slot / policy indices and the policy's shape against the pool's; policy < 0: not checked
int pool_check(hk_handle h, const char* fn, int pool, int slot, int policy)
{
    const std::string f(fn);
    if (pool < 0 || pool >= h->n_pools) return fail(h, HK_ERR_INVALID, f + ": bad pool index");
    const auto& pl = h->pool[pool];
    if (slot < 0 || slot >= pl.slots) return fail(h, HK_ERR_INVALID, f + ": bad slot index");
    if (policy == -1) return HK_OK;
    if (policy < 0 || policy >= h->n_policies) return fail(h, HK_ERR_INVALID, f + ": bad policy index");
    const int pm = h->policy[policy].lq.m;
    if (pm > 0 && pl.m == 0) return fail(h, HK_ERR_UNSUPPORTED, f + ": policy: a recurrent actor (snapshot pools of recurrent actors are out of scope)");
    if (pm == 0 && pl.m > 0) return fail(h, HK_ERR_INVALID, f + ": policy: an actor without memory (the pool holds recurrent actors: hk_policy_pool_create_recurrent)");
    const hk::PolicyParams& q = h->policy[policy].q;
    if (q.in_dim != pl.in_dim || q.stack != pl.stack || q.hidden != pl.hidden || q.n_layers != pl.n_layers || q.n_branch != pl.n_branch ||
        (q.normalize != 0) != (pl.normalize != 0))
        return fail(h, HK_ERR_INVALID, f + ": the policy's shape (in_dim, stack, hidden, n_layers, n_branch, normalize) differs from the pool's");
    if (pm != pl.m) return fail(h, HK_ERR_INVALID, f + ": the policy's memory_size differs from the pool's");
    return HK_OK;
}

inline float* pool_slot(const hk_context::Pool& pl, int slot) { return pl.buf + (size_t)slot * pl.count; }

// hk_policy_pool_create (recurrent false) and hk_policy_pool_create_recurrent: the checks, the SHAPE, the slot layout and the allocation
int pool_create(hk_handle h, const char* fn, bool recurrent, int policy, int slots)
{
    const std::string f = std::string(fn) + ": ";
    if (policy < 0 || policy >= h->n_policies) return fail(h, HK_ERR_INVALID, f + "bad policy index");
    if (slots < 1 || slots > HK_POOL_MAX_SLOTS) return fail(h, HK_ERR_INVALID, f + "slots outside [1, HK_POOL_MAX_SLOTS]");
    if (h->n_pools >= HK_MAX_POOLS) return fail(h, HK_ERR_INVALID, f + "HK_MAX_POOLS pools already exist");
    const int m = h->policy[policy].lq.m;
    if (!recurrent && m > 0) return fail(h, HK_ERR_UNSUPPORTED, f + "policy: a recurrent actor (snapshot pools of recurrent actors are out of scope)");
    if (recurrent && m == 0) return fail(h, HK_ERR_INVALID, f + "policy: an actor without memory (use hk_policy_pool_create)");
    const hk::PolicyParams& q = h->policy[policy].q;
    hk_context::Pool pl;
    pl.in_dim = q.in_dim; pl.stack = q.stack; pl.hidden = q.hidden; pl.n_layers = q.n_layers; pl.n_branch = q.n_branch; pl.normalize = q.normalize != 0;
    pl.net.layout(q.in_dim, q.hidden, q.n_layers, q.n_branch, 0);
    pl.actor = pl.net.count;
    if (recurrent) {          // the trunk through ppo_publish_kernel (a net that ends before the cell), the rest through ppo_lstm_publish_kernel: hk_ppo_publish's split
        pl.m = m;
        pl.lnet.layout(q.hidden, m, q.n_branch, pl.net.oWmu);
        pl.actor = pl.lnet.end;
        pl.net = ppo_trunk_only(pl.net, pl.lnet);          // (kept cut; ppo_publish_actor cuts whatever it is handed, which changes nothing here)
    }
    pl.slots = slots;
    pl.count = pl.actor + (pl.normalize ? 2 * (size_t)q.in_dim : 0);
    HK_HIP(h, hipMalloc(&pl.buf, (size_t)slots * pl.count * sizeof(float)));
    h->pool[h->n_pools] = pl;
    return h->n_pools++;
}

}  // namespace
}  // extern "C++"

int hk_policy_pool_create(hk_handle h, int policy, int slots)
{
    HK_NEED_ENV(h);
    return pool_create(h, "hk_policy_pool_create", false, policy, slots);
}

int hk_policy_pool_create_recurrent(hk_handle h, int policy, int slots)
{
    HK_NEED_ENV(h);
    return pool_create(h, "hk_policy_pool_create_recurrent", true, policy, slots);
}

int hk_policy_pool_count(hk_handle h, int pool)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "NULL handle");
    if (pool < 0 || pool >= h->n_pools) return fail(h, HK_ERR_INVALID, "hk_policy_pool_count: bad pool index");
    return (int)h->pool[pool].count;
}

int hk_policy_pool_save(hk_handle h, int pool, int slot, int policy)
{
    HK_NEED_ENV(h);
    if (policy == -1) policy = -2;
    int rc = pool_check(h, "hk_policy_pool_save", pool, slot, policy);
    if (rc) return rc;
    auto& pl = h->pool[pool];
    hk::PolicyDevice& pd = h->policy[policy];
    float* dst = pool_slot(pl, slot);
    ppo_publish_actor<false>(h->stream, pd, pl.net, pl.lnet, dst);
    HK_HIP(h, hipGetLastError());
    if (pl.normalize) {
        const size_t nb = (size_t)pl.in_dim * sizeof(float);
        HK_HIP(h, hipMemcpyAsync(dst + pl.actor, pd.q.mean, nb, hipMemcpyDeviceToDevice, h->stream));
        HK_HIP(h, hipMemcpyAsync(dst + pl.actor + pl.in_dim, pd.q.std, nb, hipMemcpyDeviceToDevice, h->stream));
    }
    pl.filled |= 1ull << slot;
    return HK_OK;
}

int hk_policy_pool_load(hk_handle h, int pool, int slot, int policy)
{
    HK_NEED_ENV(h);
    if (policy == -1) policy = -2;
    int rc = pool_check(h, "hk_policy_pool_load", pool, slot, policy);
    if (rc) return rc;
    const auto& pl = h->pool[pool];
    if (!((pl.filled >> slot) & 1ull)) return fail(h, HK_ERR_INVALID, "hk_policy_pool_load: the slot has never been written (hk_policy_pool_save / hk_policy_pool_put)");
    if ((rc = ppo_refuse_open(h, "hk_policy_pool_load"))) return rc;
    for (int i = 0; i < h->n_ppo; i++)
        if (h->ppo[i].policy == policy)
            return fail(h, HK_ERR_INVALID, "hk_policy_pool_load: the policy has a PPO trainer (its master weights would disagree with what plays)");
    hk::PolicyDevice& pd = h->policy[policy];
    float* src = pool_slot(pl, slot);
    ppo_publish_actor<true>(h->stream, pd, pl.net, pl.lnet, src);
    HK_HIP(h, hipGetLastError());
    if (pl.normalize) {
        const size_t nb = (size_t)pl.in_dim * sizeof(float);
        HK_HIP(h, hipMemcpyAsync(const_cast<float*>(pd.q.mean), src + pl.actor, nb, hipMemcpyDeviceToDevice, h->stream));
        HK_HIP(h, hipMemcpyAsync(const_cast<float*>(pd.q.std), src + pl.actor + pl.in_dim, nb, hipMemcpyDeviceToDevice, h->stream));
    }
    // the bf16 inference copies, when the policy has them: rebuilt from the fp32 copies just written, whichever precision the policy is in now
    if (pd.wbf) HK_HIP(h, hk::policy_bf16_refresh(pd.q, pd.bq, h->stream));
    return HK_OK;
}

int hk_policy_pool_put(hk_handle h, int pool, int slot, const float* flat)
{
    HK_NEED_ENV(h);
    int rc = pool_check(h, "hk_policy_pool_put", pool, slot, -1);
    if (rc) return rc;
    if (!flat) return fail(h, HK_ERR_INVALID, "hk_policy_pool_put: NULL pointer");
    auto& pl = h->pool[pool];
    HK_HIP(h, hipMemcpyAsync(pool_slot(pl, slot), flat, pl.count * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));          // (the host array is the caller's)
    pl.filled |= 1ull << slot;
    return HK_OK;
}

int hk_policy_pool_get(hk_handle h, int pool, int slot, float* flat)
{
    HK_NEED_ENV(h);
    int rc = pool_check(h, "hk_policy_pool_get", pool, slot, -1);
    if (rc) return rc;
    if (!flat) return fail(h, HK_ERR_INVALID, "hk_policy_pool_get: NULL pointer");
    const auto& pl = h->pool[pool];
    if (!((pl.filled >> slot) & 1ull)) return fail(h, HK_ERR_INVALID, "hk_policy_pool_get: the slot has never been written");
    HK_HIP(h, hipMemcpyAsync(flat, pool_slot(pl, slot), pl.count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_rollout_episode_stats(hk_handle h, int policy, hk_episode_stats* out)
{
    HK_NEED_ENV(h);
    const auto& ro = h->ro;
    const char* fn = "hk_rollout_episode_stats";
    if (!out) return fail(h, HK_ERR_INVALID, std::string(fn) + ": NULL pointer");
    if (policy < 0 || policy >= h->n_policies) return fail(h, HK_ERR_INVALID, std::string(fn) + ": bad policy index");
    if (!h->cfg.rewards) return fail(h, HK_ERR_INVALID, std::string(fn) + ": hk_config.rewards == 0 (the rows carry no rewards)");
    if (int rc = ppo_refuse_open(h, fn)) return rc;
    if (ro.R == 0 || !ro.buf) return fail(h, HK_ERR_INVALID, std::string(fn) + ": no rollout yet (hk_rollout_begin ... hk_rollout_close)");
    if (ro.rows < 1) return fail(h, HK_ERR_INVALID, std::string(fn) + ": the rollout closed with no completed row");
    if (policy >= ro.npol) return fail(h, HK_ERR_INVALID, std::string(fn) + ": the rollout began before the policy was attached");
    auto& ep = h->ep;
    const int E = h->cfg.num_envs, A = h->cfg.num_agents;
    const size_t ea = (size_t)E * A;
    if (!ep.buf) {
        const size_t carry_bytes = (4 * ea * 4 + 255) & ~(size_t)255;
        const size_t total = 2 * carry_bytes + (ea + 1) * sizeof(hk_episode_stats);
        HK_HIP(h, hipMalloc(&ep.buf, total));
        HK_HIP(h, hipMemsetAsync(ep.buf, 0, total, h->stream));
        for (int k = 0; k < 2; k++) {
            float* f = (float*)((char*)ep.buf + k * carry_bytes);
            ep.carry[k] = hk::EpisodeCarry{f, f + ea, (int*)(f + 2 * ea), (int*)(f + 3 * ea)};
        }
        ep.part = (hk_episode_stats*)((char*)ep.buf + 2 * carry_bytes);
        ep.out = ep.part + ea;
    }
    const hk::PolicyParams& q = h->policy[policy].q;
    hk::EpisodeRows P{};
    P.reward = ro.at<float>(HK_RO_REWARD); P.group_reward = ro.at<float>(HK_RO_GROUP_REWARD);
    P.term_reward = ro.at<float>(HK_RO_TERM_REWARD); P.term_group = ro.at<float>(HK_RO_TERM_GROUP_REWARD);
    P.done = ro.at<int>(HK_RO_DONE);
    P.R = ro.rows; P.E = E; P.A = A; P.S = q.n_slots;
    for (int j = 0; j < HK_MAX_AGENTS; j++) P.slots[j] = q.slots[j];
    const int lanes = E * q.n_slots;
    hipLaunchKernelGGL(hk::episode_scan_kernel, dim3(nblk(lanes)), dim3(256), 0, h->stream, P, ep.carry[ep.in], ep.carry_ok[policy] ? 1 : 0, ep.carry[ep.in ^ 1], ep.part);
    hipLaunchKernelGGL(hk::episode_combine_kernel, dim3(1), dim3(hk::EPISODE_COMBINE_THREADS), 0, h->stream, ep.part, lanes, ep.out);
    HK_HIP(h, hipGetLastError());
    HK_HIP(h, hipMemcpyAsync(out, ep.out, sizeof(hk_episode_stats), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    ep.stats_gen[policy] = ro.gen;
    return HK_OK;
}

int hk_obs_dim(hk_handle h)
{
    if (!h || !h->env_ready) return HK_ERR_INVALID;
    // HKA:424  Sensors.Length + sectionHorizon*5 + 8 + 12*(others + team)
    return HK_NUM_SENSORS + h->cfg.section_horizon * 5 + 8 + 12 * (h->cfg.num_agents - 1);
}

int hk_get_observations(hk_handle h, float* obs)
{
    HK_NEED_ENV(h);
    if (!obs) return fail(h, HK_ERR_INVALID, "hk_get_observations: NULL pointer");
    HK_TRY(h, hk::env_launch_observe(h->dev, h->cfg, 0xFFFFFFFFu, h->stream, h->err));
    const size_t cnt = n_karts(h) * hk_obs_dim(h);
    HK_HIP(h, hipMemcpyAsync(obs, h->dev.obs, cnt * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

// after a sync: did every env finish the ticks of the last hk_step, did an LQ solve hit a zero pivot?
static int check_device_status(hk_handle h)
{
    int st[4] = {0, 0, 0, 0};
    HK_HIP(h, hipMemcpyAsync(st, h->dev.status, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    if (st[0] & 4) {
        // reported once: the flag is cleared here (and by hk_reset), the unfinished envs keep their leftover ticks for the next hk_step
        const int keep = ~4;
        hipLaunchKernelGGL(hk::status_and_kernel, dim3(1), dim3(1), 0, h->stream, h->dev.status, keep);
        HK_HIP(h, hipGetLastError());
        return fail(h, HK_ERR_HIP, "hk_step: an env did not complete its ticks (internal scheduling error)");
    }
    return HK_OK;
}

int hk_get_agent_state(hk_handle h, hk_agent_state* out)
{
    HK_NEED_ENV(h);
    if (!out) return fail(h, HK_ERR_INVALID, "NULL pointer");
    { int rc = check_device_status(h); if (rc) return rc; }
    const size_t cnt = n_karts(h);
    // the per-tick fields live in the hot tiles (hk_env_device.h): gather them into the records first
    HK_TRY(h, hk::ga_ops(h->dev).launch_hot_gather(h->dev, h->cfg, h->stream, h->err));
    HK_HIP(h, hipMemcpyAsync(out, h->dev.agents, cnt * sizeof(hk_agent_state), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_set_agent_state(hk_handle h, const hk_agent_state* in)
{
    HK_NEED_ENV(h);
    if (h->ro.open) return fail(h, HK_ERR_INVALID, "hk_set_agent_state: refused while a rollout is open (hk_rollout_close first)");
    if (!in) return fail(h, HK_ERR_INVALID, "NULL pointer");
    const size_t cnt = n_karts(h);
    // the device divides by the section count with a multiply-shift that is exact for 0 <= x < 2^32 / L (hk_env_device.h div_L): a rewound or
    // hand-built record outside that range would index the track tables with garbage
    {
        const int64_t lim = (int64_t)(0x100000000ull / (uint64_t)std::max(1, h->cfg.num_sections)) - 2048;
        for (size_t t = 0; t < cnt; t++)
            if (in[t].section_index < 0 || in[t].init_checkpoint_index < 0 || in[t].section_index >= lim || in[t].init_checkpoint_index >= lim)
                return fail(h, HK_ERR_INVALID, "hk_set_agent_state: section_index / init_checkpoint_index out of range (negative, or beyond 2^32 / num_sections)");
    }
    h->dev.P.hold_dedupe = 0;          // the host moves karts by hand: a held kart is no longer guaranteed to be where its last solve saw it
    h->ep.moved = true;
    HK_HIP(h, hipMemcpyAsync(h->dev.agents, in, cnt * sizeof(hk_agent_state), hipMemcpyHostToDevice, h->stream));
    HK_TRY(h, hk::ga_ops(h->dev).launch_hot_scatter(h->dev, h->cfg, h->stream, h->err));
    HK_TRY(h, hk::env_mcts_invalidate(h->dev, h->cfg, h->stream, h->err));   // plans were rewritten
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_get_env_state(hk_handle h, hk_env_state* out)
{
    HK_NEED_ENV(h);
    if (!out) return fail(h, HK_ERR_INVALID, "NULL pointer");
    { int rc = check_device_status(h); if (rc) return rc; }
    HK_TRY(h, hk::ga_ops(h->dev).launch_envs_gather(h->dev, h->cfg, h->stream, h->err));
    HK_HIP(h, hipMemcpyAsync(out, h->dev.envs_stage, (size_t)h->cfg.num_envs * sizeof(hk_env_state), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_set_env_state(hk_handle h, const hk_env_state* in)
{
    HK_NEED_ENV(h);
    if (h->ro.open) return fail(h, HK_ERR_INVALID, "hk_set_env_state: refused while a rollout is open (hk_rollout_close first)");
    if (!in) return fail(h, HK_ERR_INVALID, "NULL pointer");
    h->dev.P.hold_dedupe = 0;          // (as hk_set_agent_state: episode_steps may be rewound into a hold whose solves were skipped)
    h->lock_tick = -1;                 // (the host wrote episode steps)
    h->ep.moved = true;
    HK_HIP(h, hipMemcpyAsync(h->dev.envs_stage, in, (size_t)h->cfg.num_envs * sizeof(hk_env_state), hipMemcpyHostToDevice, h->stream));
    HK_TRY(h, hk::ga_ops(h->dev).launch_envs_scatter(h->dev, h->cfg, h->stream, h->err));   // (progress words sanitized on the way)
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_get_episode_results(hk_handle h, hk_episode_result* out)
{
    HK_NEED_ENV(h);
    if (!out) return fail(h, HK_ERR_INVALID, "NULL pointer");
    const size_t cnt = n_karts(h);
    HK_HIP(h, hipMemcpyAsync(out, h->dev.results, cnt * sizeof(hk_episode_result), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_comm_unique_id(void* id_out)
{
    if (!id_out) return fail(nullptr, HK_ERR_INVALID, "hk_comm_unique_id: NULL pointer");
    std::string err;
    if (!g_rccl.load(err)) return fail(nullptr, HK_ERR_UNSUPPORTED, err);
    RcclId id;
    const int rc = g_rccl.GetUniqueId(&id);
    if (rc != 0) return fail(nullptr, HK_ERR_HIP, "ncclGetUniqueId: " + g_rccl.why(rc));
    std::memcpy(id_out, id.internal, HK_COMM_ID_BYTES);
    return HK_OK;
}

int hk_comm_init(hk_handle h, int world_size, int rank, const void* id)
{
    HK_NEED_ENV(h);
    if (!id || world_size < 1 || rank < 0 || rank >= world_size) return fail(h, HK_ERR_INVALID, "hk_comm_init: bad world_size / rank / id");
    if (h->comm) return fail(h, HK_ERR_INVALID, "hk_comm_init: this handle already has a communicator");
    if (!g_rccl.load(h->err)) return hand_off(h, HK_ERR_UNSUPPORTED);
    RcclId rid;
    std::memcpy(rid.internal, id, HK_COMM_ID_BYTES);
    const int rc = g_rccl.CommInitRank(&h->comm, world_size, rid, rank);
    if (rc != 0) { h->comm = nullptr; return fail(h, HK_ERR_HIP, "ncclCommInitRank: " + g_rccl.why(rc)); }
    h->comm_world = world_size; h->comm_rank = rank;
    return HK_OK;
}

// The size exchange of both gathers: this rank's word `mine` out, every rank's word (rank order) back in `all`; synchronises the handle's stream.
// gather_cnt holds the W gathered words and, behind them, this rank's own.
static int gather_words(hk_handle h, unsigned long long mine, std::vector<unsigned long long>& all)
{
    const int W = h->comm_world;
    const size_t bytes = (size_t)W * sizeof(mine);
    if (int rc = dev_grow(h, &h->gather_cnt, &h->gather_cnt_bytes, bytes + sizeof(mine), bytes + sizeof(mine))) return rc;
    unsigned long long* d_cnt = (unsigned long long*)h->gather_cnt;
    HK_HIP(h, hipMemcpyAsync(d_cnt + W, &mine, sizeof(mine), hipMemcpyHostToDevice, h->stream));
    const int rc = g_rccl.AllGather(d_cnt + W, d_cnt, sizeof(mine), /*ncclChar*/ 0, h->comm, h->stream);
    if (rc != 0) return fail(h, HK_ERR_HIP, "ncclAllGather (sizes): " + g_rccl.why(rc));
    all.resize((size_t)W);
    HK_HIP(h, hipMemcpyAsync(all.data(), d_cnt, bytes, hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_gather_results(hk_handle h, hk_episode_result* all)
{
    HK_NEED_ENV(h);
    if (!all) return fail(h, HK_ERR_INVALID, "hk_gather_results: NULL pointer");
    if (!h->comm) return fail(h, HK_ERR_INVALID, "hk_gather_results: call hk_comm_init first");
    { int rc = check_device_status(h); if (rc) return rc; }
    const int W = h->comm_world;
    const size_t local = n_karts(h) * sizeof(hk_episode_result);
    // Ranks may hold different env counts (a contiguous split of a total that the world size does not divide): exchange the
    // byte counts first (8 bytes per rank), pad every contribution to the largest, gather, and trim on the way to the host.
    std::vector<unsigned long long> cnt;
    if (int rc = gather_words(h, (unsigned long long)local, cnt)) return rc;
    size_t per = 0;
    for (int r = 0; r < W; r++) {
        if (cnt[r] % ((size_t)h->cfg.num_agents * sizeof(hk_episode_result)) != 0)
            return fail(h, HK_ERR_INVALID, "hk_gather_results: a rank holds a different num_agents");
        per = cnt[r] > per ? (size_t)cnt[r] : per;
    }
    const size_t total = per * (size_t)W + per;                              // [W] padded slots + this rank's padded send slot
    if (int rc = dev_grow(h, &h->gather_buf, &h->gather_bytes, total, total)) return rc;
    char* buf = (char*)h->gather_buf;
    const void* send = h->dev.results;
    if (local < per) {                                                       // pad this rank's contribution
        HK_HIP(h, hipMemsetAsync(buf + per * W, 0, per, h->stream));
        HK_HIP(h, hipMemcpyAsync(buf + per * W, h->dev.results, local, hipMemcpyDeviceToDevice, h->stream));
        send = buf + per * W;
    }
    // bytes on the wire (ncclChar): the records are plain data, identical layout on every rank
    const int rc = g_rccl.AllGather(send, buf, per, /*ncclChar*/ 0, h->comm, h->stream);
    if (rc != 0) return fail(h, HK_ERR_HIP, "ncclAllGather: " + g_rccl.why(rc));
    char* out = (char*)all;
    for (int r = 0; r < W; r++) {                                            // rank r's rows, trimmed to what it holds
        if (cnt[r]) HK_HIP(h, hipMemcpyAsync(out, buf + per * r, (size_t)cnt[r], hipMemcpyDeviceToHost, h->stream));
        out += cnt[r];
    }
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_gather_count(hk_handle h, int64_t* total_envs)
{
    HK_NEED_ENV(h);
    if (!total_envs) return fail(h, HK_ERR_INVALID, "hk_gather_count: NULL pointer");
    if (!h->comm) return fail(h, HK_ERR_INVALID, "hk_gather_count: call hk_comm_init first");
    const int W = h->comm_world;
    std::vector<unsigned long long> cnt;
    if (int rc = gather_words(h, (unsigned long long)h->cfg.num_envs, cnt)) return rc;
    int64_t t = 0;
    for (int r = 0; r < W; r++) t += (int64_t)cnt[r];
    *total_envs = t;
    return HK_OK;
}

int hk_comm_destroy(hk_handle h)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "NULL handle");
    if (h->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(h->comm);
    h->comm = nullptr; h->comm_world = 0;
    return HK_OK;
}

int hk_get_rewards(hk_handle h, float* reward, float* group_reward)
{
    HK_NEED_ENV(h);
    if (h->ro.open) return fail(h, HK_ERR_INVALID, "hk_get_rewards: refused while a rollout is open (hk_rollout_close first)");
    if (!reward || !group_reward) return fail(h, HK_ERR_INVALID, "NULL pointer");
    { int rc = check_device_status(h); if (rc) return rc; }
    const size_t cnt = n_karts(h);
    float* d_r = h->dev.reward_out;
    HK_TRY(h, hk::ga_ops(h->dev).launch_rewards_read(h->dev, (int)cnt, d_r, d_r + cnt, h->stream, h->err));
    HK_HIP(h, hipMemcpyAsync(reward, d_r, cnt * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipMemcpyAsync(group_reward, d_r + cnt, cnt * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_get_mcts_state(hk_handle h, hk_mcts_state* out)
{
    HK_NEED_ENV(h);
    if (!out) return fail(h, HK_ERR_INVALID, "NULL pointer");
    { int rc = check_device_status(h); if (rc) return rc; }
    const size_t cnt = n_karts(h);
    if (!h->dev.mcts.st) { std::memset(out, 0, cnt * sizeof(hk_mcts_state)); return HK_OK; }
    if (h->dev.mcts_ticks > 0) {          // searches deferred by short hk_step calls: `pend` must be there when the host looks
        HK_TRY(h, hk::env_flush_mcts(h->dev, h->stream, h->err));
    }
    HK_HIP(h, hipMemcpyAsync(out, h->dev.mcts.st, cnt * sizeof(hk_mcts_state), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

int hk_get_lq_debug(hk_handle h, int env, int ego, hk_lq_debug* out)
{
    HK_NEED_ENV(h);
    if (!out || env < 0 || env >= h->cfg.num_envs || ego < 0 || ego >= h->cfg.num_agents)
        return fail(h, HK_ERR_INVALID, "hk_get_lq_debug: bad arguments");
    if (!h->dev.lq_debug) return fail(h, HK_ERR_INVALID, "hk_get_lq_debug: debug taps are off");
    HK_HIP(h, hipMemcpyAsync(out, h->dev.lq_debug + ((size_t)env * h->cfg.num_agents + ego), sizeof(hk_lq_debug),
                             hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

// The device-pointer getters hand out the library's own buffers for zero-copy consumers (torch, the C# host's compute buffers).  Each one first SETTLES
// the handle like every other getter — laggards of a lazily completed call, the completion guard of optimistic short calls, a search launch on the
// planner's side stream — so that what the pointer shows, once the handle's stream has been synchronised, is the state hk_synchronize would leave.
// The work is issued on the handle's stream; a pointer taken BEFORE a later hk_step shows that step's results only after the next getter / hk_synchronize.
// (a NULL handle or one without an environment leaves the messages alone, as the pointer getters below do)
static bool settle_for_pointer(hk_handle h) { return h && h->env_ready && settle(h, SETTLE_ALL) == HK_OK; }
void* hk_device_results_ptr(hk_handle h) { return settle_for_pointer(h) ? (void*)h->dev.results : nullptr; }
void* hk_device_agents_ptr(hk_handle h)
{
    // a SNAPSHOT: the per-tick fields are gathered from the hot tiles into the records (asynchronously, on the handle's stream) by this call;
    // after further hk_step calls the pointer has to be requested again
    if (!settle_for_pointer(h)) return nullptr;
    if (hand_off(h, hk::ga_ops(h->dev).launch_hot_gather(h->dev, h->cfg, h->stream, h->err)) != HK_OK) return nullptr;
    return (void*)h->dev.agents;
}
void* hk_device_obs_ptr(hk_handle h) { return settle_for_pointer(h) ? (void*)h->dev.obs : nullptr; }
void* hk_device_act_steer_ptr(hk_handle h) { return (h && h->env_ready) ? (void*)h->dev.act_steer : nullptr; }
void* hk_device_act_branch_ptr(hk_handle h) { return (h && h->env_ready) ? (void*)h->dev.act_branch : nullptr; }
void* hk_device_reward_ptr(hk_handle h) { return (h && h->env_ready) ? (void*)h->dev.reward_out : nullptr; }
void* hk_device_group_reward_ptr(hk_handle h)
{
    return (h && h->env_ready && h->dev.reward_out) ? (void*)(h->dev.reward_out + n_karts(h)) : nullptr;
}

int hk_observe(hk_handle h)
{
    HK_NEED_ENV(h);
    return hand_off(h, hk::env_launch_observe(h->dev, h->cfg, 0xFFFFFFFFu, h->stream, h->err));
}

int hk_rewards_device(hk_handle h)
{
    HK_NEED_ENV(h);
    if (h->ro.open) return fail(h, HK_ERR_INVALID, "hk_rewards_device: refused while a rollout is open (hk_rollout_close first)");
    const size_t cnt = n_karts(h);
    return hand_off(h, hk::ga_ops(h->dev).launch_rewards_read(h->dev, (int)cnt, h->dev.reward_out, h->dev.reward_out + cnt, h->stream, h->err));
}

int hk_prof_enable(hk_handle h, int on)
{
    if (!h) return HK_ERR_INVALID;
    HK_HIP(h, hipSetDevice(h->device));
    h->prof.on = on != 0;
    return HK_OK;
}

int hk_prof_reset(hk_handle h)
{
    if (int rc = settle(h, SETTLE_PROF)) return rc;
    HK_HIP(h, hipStreamSynchronize(h->stream));
    h->prof.fold();
    for (int s = 0; s < HK_PROF_STAGES; s++) { h->prof.ms[s] = 0; h->prof.n[s] = 0; }
    if (h->env_ready && h->dev.game_stats) {
        HK_HIP(h, hipMemsetAsync(h->dev.game_stats, 0, hk::GAME_METER * sizeof(unsigned long long), h->stream));      // (not the games-per-launch meter behind the statistics: the schedule lives on it)
        HK_HIP(h, hipStreamSynchronize(h->stream));
    }
    return HK_OK;
}

int hk_prof_games(hk_handle h, int64_t* games)
{
    HK_NEED_ENV(h);
    if (!games) return fail(h, HK_ERR_INVALID, "hk_prof_games: NULL pointer");
    unsigned long long g[hk::GAME_STATS_N];
    HK_HIP(h, hipMemcpyAsync(g, h->dev.game_stats, sizeof(g), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    for (int n = 0; n <= HK_MAX_AGENTS; n++) games[n] = (int64_t)g[n];
#ifdef HK_STAMPS
    {       // diagnostic builds (-DHK_STAMPS): the phase cycle counters of the tick kernel
        std::fprintf(stderr, "HK_STAMPS");
        for (int k = 16; k < hk::GAME_STATS_N; k++) std::fprintf(stderr, " %llu", g[k]);
        std::fprintf(stderr, "\n");
    }
#endif
    return HK_OK;
}

int hk_prof_meter(hk_handle h, int64_t* words)
{
    HK_NEED_ENV(h);
    if (!words) return fail(h, HK_ERR_INVALID, "hk_prof_meter: NULL pointer");
    static_assert(HK_METER_PARTS == hk::GAME_METER_PARTS, "hk.h HK_METER_PARTS");
    unsigned long long m[4 * hk::GAME_METER_PARTS];
    HK_HIP(h, hipMemcpyAsync(m, h->dev.game_stats + hk::GAME_METER, sizeof(m), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < 4 * hk::GAME_METER_PARTS; k++) words[k] = (int64_t)m[k];
    return HK_OK;
}

int hk_prof_read(hk_handle h, double* ms, int64_t* launches)
{
    if (int rc = settle(h, SETTLE_PROF)) return rc;
    HK_HIP(h, hipStreamSynchronize(h->stream));
    h->prof.fold();
    for (int s = 0; s < HK_PROF_STAGES; s++) {
        if (ms) ms[s] = h->prof.ms[s];
        if (launches) launches[s] = h->prof.n[s];
    }
    return HK_OK;
}

}  // extern "C"
