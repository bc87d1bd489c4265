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
#define HK_POLICY_KERNELS      // this unit is the one that defines the actor kernels of hk_policy.h / _bf16.h / _lstm.h and their launchers
#include "../../include/hk.h"
#include "hk_lq_core.h"
#include "hk_env_kernels.h"
#include "hk_policy.h"
#include "hk_handle.h"
#include "hk_rollout.h"
#include "hk_selfplay.h"
#include <dlfcn.h>

namespace hk {
// hk_lq_batch.hip
int lq_batch_launch(int batch, int N, const double* dA, const double* dB, const double* dQ, const double* dq, const double* dR,
                    const double* dx0, int horizon, double* du0, int* d_status, hipStream_t st);
}
thread_local std::string hk::g_last_error;      // what hk_last_error(NULL) returns: fail and hand_off (hk_handle.h) write it, in both units

static int finish_ticks(hk_context* h);      // lazy completion of the last hk_step (defined with step_ticks)
static int meter_copy(hk_context* h, bool in_order);      // the games-per-launch meter on its way to pinned memory (defined with step_ticks)
static int throttle_mark(hk_context* h, int r);           // long lazy calls: stay a bounded number of rounds ahead of the GPU, look at the meter (defined with step_ticks)
static int verify_optimistic(hk_context* h); // the completion guard of optimistic fixed-round calls, looked at; laggards finished (defined with step_ticks)
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
}  // namespace
int hk::settle_all(hk_context* h) { return settle(h, SETTLE_ALL); }      // the trainers' HK_NEED_ENV (hk_train.hip)
namespace {

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

const char* hk_last_error(hk_handle h) { return h ? h->err.c_str() : hk::g_last_error.c_str(); }

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
    if (rc) { hk::g_last_error = h->err; delete h; return rc; }
    h->tune.read();
    if (!(h->train = hk::train_create())) { hk_destroy(h); return fail(nullptr, HK_ERR_INVALID, "hk_create: out of memory"); }
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
        if (rc) { hk::g_last_error = h->err; hk_destroy(h); return rc; }
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
    hk::train_destroy(h);
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

// hk_policy_set_precision for a policy with memory (hk.h "RECURRENT ACTORS IN BF16"): the trunk's copies as above, and the cell's beside them
int hk_policy_lstm_set_precision(hk_handle h, int policy, int precision)
{
    HK_NEED_ENV(h);
    if (policy < 0 || policy >= h->n_policies) return fail(h, HK_ERR_INVALID, "hk_policy_lstm_set_precision: bad policy index");
    if (precision != HK_POLICY_PREC_F32 && precision != HK_POLICY_PREC_BF16) return fail(h, HK_ERR_INVALID, "hk_policy_lstm_set_precision: unknown precision");
    if (h->ro.open) return fail(h, HK_ERR_INVALID, "hk_policy_lstm_set_precision: refused while a rollout is open (hk_rollout_close first)");
    hk::PolicyDevice& pd = h->policy[policy];
    if (pd.lq.m == 0) return fail(h, HK_ERR_INVALID, "hk_policy_lstm_set_precision: the policy has no memory (use hk_policy_set_precision)");
    if (precision == HK_POLICY_PREC_BF16 && !pd.wlbf) {
        // one allocation for the trunk's and one for the cell's fragment-major bf16 copies, built on the stream from the CURRENT fp32 copies
        size_t off[HK_POLICY_MAX_LAYERS + 1] = {};
        for (int l = 0; l < pd.q.n_layers; l++) off[l + 1] = off[l] + hk::policy_bf16_layer_elems(pd.q, l);
        const size_t n_ih = hk::policy_lstm_bf16_ih_elems(pd.q, pd.lq), n_hh = hk::policy_lstm_bf16_hh_elems(pd.lq);
        uint16_t *wbf = nullptr, *wlbf = nullptr;
        hipError_t e = hipMalloc(&wbf, off[pd.q.n_layers] * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMalloc(&wlbf, (n_ih + n_hh) * sizeof(uint16_t));
        hk::PolicyBf16 bq{};
        for (int l = 0; l < pd.q.n_layers; l++) bq.Wf[l] = wbf + off[l];
        const hk::PolicyLstmBf16 lbq{wlbf, wlbf + n_ih};
        if (e == hipSuccess) e = hk::policy_bf16_refresh(pd.q, bq, h->stream);
        if (e == hipSuccess) e = hk::policy_lstm_bf16_refresh(pd.q, pd.lq, lbq, h->stream);
        if (e != hipSuccess) {
            (void)hipFree(wbf);
            (void)hipFree(wlbf);
            HK_HIP(h, e);
        }
        pd.wbf = wbf; pd.bq = bq;
        pd.wlbf = wlbf; pd.lbq = lbq;
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

// the episode statistics of self-play (hk.h "SELF-PLAY"; device side in hk_selfplay.h); the trainers and the snapshot pools: hk_train.hip
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
