// hk_train.hip — the trainers and the snapshot pools of the C ABI (include/hk.h): PPO in both precisions, POCA, recurrent PPO with and without
// a recurrent critic, the running normaliser, the long-run options, hk_policy_pool_*.  The handle, the error hand-off and the buffer helpers are
// hk_handle.h's; the environment's entry points, the actors' kernels and the rollout recorder are hk_api.hip's, and nothing here knows the scheduler.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <new>
#include "../../include/hk.h"
#include "hk_handle.h"
#include "hk_ppo.h"
#include "hk_ppo_lstm.h"
#include "hk_ppo_lstm_bf16.h"
#include "hk_ppo_lstm_critic.h"
#include "hk_poca.h"

#define HK_NEED_ENV(h) do { if (int rc_ = hk::settle_all(h)) return rc_; } while (0)

// PPO trainers (hk_ppo_*; hk_ppo.h): a master copy of the actor + critic parameters, Adam moments, the rollout's per-row values, and a
// workspace sized by the largest minibatch seen
struct hk_context::Ppo {
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
};

// self-play (hk.h "SELF-PLAY"): a snapshot pool; nothing is allocated before the first hk_policy_pool_create
struct hk_context::Pool {
    int in_dim = 0, stack = 0, hidden = 0, n_layers = 0, n_branch = 0, normalize = 0;    // the SHAPE
    hk::PpoNet net;                // the flat actor layout (base 0); a slot is net.count floats, then mean, std [in_dim] when normalize
    int m = 0;                     // > 0: a recurrent pool (hk_policy_pool_create_recurrent) of memory_size 2m; net is then the trunk alone
    hk::PpoLstmNet lnet;           // (it ends at lnet.oWih) and lnet the cell and the m-wide heads behind it; the actor is lnet.end floats
    size_t actor = 0;              // floats of the actor part of a slot: net.count, or lnet.end for a recurrent pool
    int slots = 0;
    size_t count = 0;              // floats per slot
    float* buf = nullptr;          // [slots][count]
    uint64_t filled = 0;           // bit s: slot s has been written
};

struct hk::TrainState {
    hk_context::Ppo ppo[HK_MAX_POLICIES];
    int n_ppo = 0;
    hk_context::Pool pool[HK_MAX_POOLS];
    int n_pools = 0;
};

static void ppo_release(hk_context::Ppo& t); // every device allocation of a trainer freed, the slot empty again (defined with the PPO trainer)

extern "C" {

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
    // (a recurrent actor's last post-activation is bf16 too: it is an operand of the cell's product and no head reads it)
    for (int l = 0; l < t.actor.n_layers; l++) { d.Za[l] = fl(Mz * Ha); d.Aa[l] = mat(Mz * Ha, bf && (l < t.actor.n_layers - 1 || t.seq_len)); }
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
    uint16_t *GZb, *hprevb;          // HK_PPO_PREC_BF16 (the actor's cell): the gate deltas and h_prev as the products read them; nullptr otherwise
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
    if (!critic && t.prec == HK_PPO_PREC_BF16) { d.GZb = (uint16_t*)a.take(Mz * 4 * mc * 2); d.hprevb = (uint16_t*)a.take(Mz * mc * 2); }
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
    ppo_product<0>(s, M, 4 * c.m, c.H, A, c.H, true, ppo_weights(t, c.oWih), c.H, true, bsum, PpoMat(Zx), 4 * c.m, nullptr, c.H);
}

// step tau of a cell's forward over ms rows: GZ's Zx continued over h with W_hh (of h's kind: the step kernel of that precision), then the cell.
// htap (hk_ppo_lstm_gates_bf16 only): h as given, no cell, GZ returns the pre-activations
void ppo_cell_step(hipStream_t s, int tau, int ms, int m, PpoMat Whh, const PpoLstmWs& r, const int* first, const uint16_t* htap = nullptr)
{
    if (Whh.b)
        hipLaunchKernelGGL(hk::ppo_lstm_step_bf16_kernel, dim3(nblk(m, hk::PB_TN), nblk(ms, hk::PB_TM)), dim3(256), 0, s, tau, ms, m, Whh.b, r.mem0, first, htap,
                           r.GZ, r.hnew, r.mbmem, r.hprev, r.hprevb, r.cprev);
    else
        hipLaunchKernelGGL(hk::ppo_lstm_step_kernel, dim3(nblk(m, hk::PPO_TN), nblk(ms, hk::PPO_TM)), dim3(256), 0, s, tau, ms, m, Whh.f, r.mem0, first, r.GZ,
                           r.hnew, r.mbmem, r.hprev, r.cprev);
}

// a cell's forward over a minibatch's ms windows (M = L ms time-major rows) in its workspace r: the input projection over all rows at once, then
// the L steps from r.mem0
void ppo_cell_forward(hipStream_t s, const hk_context::Ppo& t, const PpoCell& c, const PpoLstmWs& r, PpoMat A, const int* first, int ms)
{
    const int L = t.seq_len;
    ppo_cell_bsum(s, t, c, r.bsum);
    ppo_cell_project(s, t, c, L * ms, A, r.bsum, r.GZ);
    const PpoMat Whh = A.b ? ppo_weights(t, c.oWhh) : PpoMat(t.param + c.oWhh);
    for (int tau = 0; tau < L; tau++) ppo_cell_step(s, tau, ms, c.m, Whh, r, first);
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
    // the gate deltas, h_prev and the cell's weights as the products read them: of A[top]'s kind (bf16: rounded once by the kernels that make them)
    const bool bf = A[top].b != nullptr;
    const PpoMat dG = bf ? PpoMat(r.GZb) : PpoMat(r.GZ), hp = bf ? PpoMat(r.hprevb) : PpoMat(r.hprev);
    const PpoMat Wih = bf ? ppo_weights(t, c.oWih) : PpoMat(prm + c.oWih), Whh = bf ? ppo_weights(t, c.oWhh) : PpoMat(prm + c.oWhh);
    auto at = [](PpoMat x, size_t o) { return x.b ? PpoMat(x.b + o) : PpoMat(x.f + o); };
    for (int tau = L - 1; tau >= 0; tau--) {
        const dim3 grid(nblk((size_t)ms * m));
        if (bf)
            hipLaunchKernelGGL(hk::ppo_lstm_back_bf16_kernel, grid, dim3(256), 0, s, tau, ms, m, (int)(tau == L - 1), first, r.dH, r.drec, r.mbmem, r.cprev, r.GZ,
                               r.GZb, r.dcar);
        else
            hipLaunchKernelGGL(hk::ppo_lstm_back_kernel, grid, dim3(256), 0, s, tau, ms, m, (int)(tau == L - 1), first, r.dH, r.drec, r.mbmem, r.cprev, r.GZ, r.dcar);
        if (tau > 0)          // the recurrent delta to tau - 1: dG_tau [ms][4m] W_hh [4m][m]
            ppo_product<0>(s, ms, m, N, at(dG, (size_t)tau * ms * N), N, true, Whh, m, false, nullptr, PpoMat(r.drec), m, nullptr, N);
    }
    ppo_wgrad(s, r.part, N, H, M, dG, N, A[top], H, grad + c.oWih, nullptr);
    ppo_wgrad(s, r.part, N, m, M, dG, N, hp, m, grad + c.oWhh, nullptr);
    ppo_colsum(s, dG, M, N, N, grad + c.obih);
    HK_HIP(h, hipMemcpyAsync(grad + c.obhh, grad + c.obih, (size_t)N * sizeof(float), hipMemcpyDeviceToDevice, s));      // both biases: the same gradient
    ppo_product<2>(s, M, H, N, dG, N, true, Wih, H, false, nullptr, w.d0, H, Z[top], N);
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

int ppo_check(hk_handle h, int trainer, const char* fn, bool need_adv)
{
    if (trainer < 0 || trainer >= h->train->n_ppo) return fail(h, HK_ERR_INVALID, std::string(fn) + ": bad trainer index");
    const auto& t = h->train->ppo[trainer];
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
    const auto& t = h->train->ppo[trainer];
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
    for (int i = 0; i < h->train->n_ppo; i++) if (h->train->ppo[i].policy == policy) h->train->ppo[i].adv_stale = true;
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
    if (h->train->n_ppo >= HK_MAX_POLICIES) return fail(h, HK_ERR_INVALID, f + "HK_MAX_POLICIES trainers already exist");
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
    auto& t = h->train->ppo[h->train->n_ppo];
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
    return h->train->n_ppo++;
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
    auto& t = h->train->ppo[idx];
    const size_t each = ppo_critic_mem(h, t).each;
    hipError_t e = hipMalloc(&t.cmem, 3 * each * sizeof(float));
    if (e == hipSuccess) e = hipMemsetAsync(t.cmem, 0, 3 * each * sizeof(float), h->stream);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)hk::ppo_lstm_value_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {          // (give the slot back)
        ppo_release(t);
        h->train->n_ppo--;
        return fail(h, HK_ERR_HIP, f + hipGetErrorString(e));
    }
    return idx;
}

int hk_ppo_advantages(hk_handle h, int trainer)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_advantages", false);
    if (rc) return rc;
    auto& t = h->train->ppo[trainer];
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
    auto& t = h->train->ppo[trainer];
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
    return ppo_adam_step(h, h->train->ppo[trainer], lr);
}

int hk_ppo_publish(hk_handle h, int trainer)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_publish", false);
    if (rc) return rc;
    if ((rc = ppo_refuse_open(h, "hk_ppo_publish"))) return rc;
    auto& t = h->train->ppo[trainer];
    hk::PolicyDevice& pd = h->policy[t.policy];
    ppo_publish_actor<true>(h->stream, pd, t.actor, t.lnet, t.param);
    HK_HIP(h, hipGetLastError());
    // the bf16 inference copies, when a plain actor's policy has them: rebuilt from the fp32 copies just written (each an exact copy of its master,
    // so every weight is the master rounded once by ppo_bf16_rne: HK_PPO_SHADOW's element), whichever precision the policy is in now
    if (!t.seq_len && pd.wbf) HK_HIP(h, hk::policy_bf16_refresh(pd.q, pd.bq, h->stream));
    // ... and a recurrent actor's (hk_policy_lstm_set_precision made them): the trunk's and the cell's
    if (t.seq_len && pd.wlbf) {
        HK_HIP(h, hk::policy_bf16_refresh(pd.q, pd.bq, h->stream));
        HK_HIP(h, hk::policy_lstm_bf16_refresh(pd.q, pd.lq, pd.lbq, h->stream));
    }
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
    auto& t = h->train->ppo[trainer];
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
    return ppo_adam_step(h, h->train->ppo[trainer], lr, max_grad_norm);
}

int hk_ppo_get_counters(hk_handle h, int trainer, int64_t* adam_steps, int64_t* epochs_done)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_get_counters", false);
    if (rc) return rc;
    const auto& t = h->train->ppo[trainer];
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
    auto& t = h->train->ppo[trainer];
    t.adam_steps = (int)adam_steps; t.epochs_done = (int)epochs_done;
    return HK_OK;
}

int hk_ppo_normalizer_init(hk_handle h, int trainer, int64_t steps)
{
    HK_NEED_ENV(h);
    int rc = ppo_norm_check(h, trainer, "hk_ppo_normalizer_init", false);
    if (rc) return rc;
    auto& t = h->train->ppo[trainer];
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
    auto& t = h->train->ppo[trainer];
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
    const auto& t = h->train->ppo[trainer];
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
    auto& t = h->train->ppo[trainer];
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

// the switch itself, after the entry point's refusals (hk_ppo_set_precision, hk_ppo_recurrent_set_precision)
static int ppo_switch_precision(hk_handle h, hk_context::Ppo& t, int precision)
{
    if (precision == t.prec) return HK_OK;
    // the workspace is laid out per precision: drop it once the stream is done with it (the next minibatch allocates the other layout)
    HK_HIP(h, hipStreamSynchronize(h->stream));
    t.cap = 0; t.last_m = 0;
    HK_HIP(h, dev_free(t.ws));
    if (t.seq_len) { t.rcap = 0; t.last_ms = 0; HK_HIP(h, dev_free(t.rws)); }          // (a recurrent trainer's cell workspace likewise)
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

int hk_ppo_set_precision(hk_handle h, int trainer, int precision)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_set_precision", false);
    if (rc) return rc;
    if (precision != HK_PPO_PREC_F32 && precision != HK_PPO_PREC_BF16) return fail(h, HK_ERR_INVALID, "hk_ppo_set_precision: unknown precision");
    auto& t = h->train->ppo[trainer];
    if (t.poca && precision != HK_PPO_PREC_F32) return fail(h, HK_ERR_UNSUPPORTED, "hk_ppo_set_precision: a POCA trainer has no bf16 products (hk.h \"POCA\")");
    if (t.seq_len && precision != HK_PPO_PREC_F32)
        return fail(h, HK_ERR_UNSUPPORTED, "hk_ppo_set_precision: precision: a recurrent trainer has no bf16 products (hk.h \"PPO trainer\" RECURRENT)");
    return ppo_switch_precision(h, t, precision);
}

int hk_ppo_get_precision(hk_handle h, int trainer)
{
    if (!h) return fail(nullptr, HK_ERR_INVALID, "NULL handle");
    if (trainer < 0 || trainer >= h->train->n_ppo) return fail(h, HK_ERR_INVALID, "hk_ppo_get_precision: bad trainer index");
    return h->train->ppo[trainer].prec;
}

// hk_ppo_set_precision for a trainer made by hk_ppo_create_recurrent (hk.h "RECURRENT ACTORS IN BF16")
int hk_ppo_recurrent_set_precision(hk_handle h, int trainer, int precision)
{
    HK_NEED_ENV(h);
    int rc = ppo_check(h, trainer, "hk_ppo_recurrent_set_precision", false);
    if (rc) return rc;
    if (precision != HK_PPO_PREC_F32 && precision != HK_PPO_PREC_BF16) return fail(h, HK_ERR_INVALID, "hk_ppo_recurrent_set_precision: unknown precision");
    auto& t = h->train->ppo[trainer];
    if (!t.seq_len) return fail(h, HK_ERR_INVALID, "hk_ppo_recurrent_set_precision: the trainer is not recurrent (use hk_ppo_set_precision)");
    if (t.critic_m)
        return fail(h, HK_ERR_UNSUPPORTED, "hk_ppo_recurrent_set_precision: a trainer with a recurrent critic has no bf16 products (the critic's cell is fp32)");
    return ppo_switch_precision(h, t, precision);
}

// a debug tap: the recurrent bf16 trainer's own two launches of the gate pre-activations on the caller's device buffers
int hk_ppo_lstm_gates_bf16(hk_handle h, int rows, int H, int m, const void* a_dev, const void* h_dev, const void* W_ih_dev, const void* W_hh_dev, const float* bsum_dev,
                           float* z_dev)
{
    HK_NEED_ENV(h);
    if (rows < 1 || H < 1 || m < 1) return fail(h, HK_ERR_INVALID, "hk_ppo_lstm_gates_bf16: rows, H, m must be positive");
    if (H % 32 || m % 32) return fail(h, HK_ERR_INVALID, "hk_ppo_lstm_gates_bf16: H and m must be multiples of 32");
    if ((long long)rows * 4 * m > 0x3FFFFFFF) return fail(h, HK_ERR_INVALID, "hk_ppo_lstm_gates_bf16: rows x 4m elements do not fit");
    if (!a_dev || !h_dev || !W_ih_dev || !W_hh_dev || !bsum_dev || !z_dev) return fail(h, HK_ERR_INVALID, "hk_ppo_lstm_gates_bf16: NULL operand");
    hipStream_t s = h->stream;
    // Zx = bsum + a W_ih^T (ppo_cell_project's product), then one step's chains over h without the cell (ppo_cell_step)
    ppo_product<0>(s, rows, 4 * m, H, PpoMat((uint16_t*)a_dev), H, true, PpoMat((uint16_t*)W_ih_dev), H, true, bsum_dev, PpoMat(z_dev), 4 * m, nullptr, H);
    PpoLstmWs r{};
    r.GZ = z_dev;
    ppo_cell_step(s, 0, rows, m, PpoMat((uint16_t*)W_hh_dev), r, nullptr, (const uint16_t*)h_dev);
    HK_HIP(h, hipGetLastError());
    return HK_OK;
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
    if (trainer < 0 || trainer >= h->train->n_ppo) { fail(h, HK_ERR_INVALID, "hk_ppo_ptr: bad trainer index"); return nullptr; }
    const auto& t = h->train->ppo[trainer];
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
    if (trainer < 0 || trainer >= h->train->n_ppo) return fail(h, HK_ERR_INVALID, "hk_ppo_count: bad trainer index");
    const auto& t = h->train->ppo[trainer];
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
    if (trainer < 0 || trainer >= h->train->n_ppo) return fail(h, HK_ERR_INVALID, std::string(fn) + ": bad trainer index");
    if (!h->train->ppo[trainer].poca) return fail(h, HK_ERR_INVALID, std::string(fn) + ": not a POCA trainer (hk_ppo_create_poca)");
    if (field < 0 || field >= HK_POCA_FIELDS) return fail(h, HK_ERR_INVALID, std::string(fn) + ": bad field");
    return HK_OK;
}
}  // namespace
}  // extern "C++"

void* hk_poca_ptr(hk_handle h, int trainer, int field)
{
    if (poca_field_check(h, trainer, field, "hk_poca_ptr")) return nullptr;
    const auto& t = h->train->ppo[trainer];
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
    const auto& t = h->train->ppo[trainer];
    if (field == HK_POCA_MB_BASELINE) return t.last_m;
    return t.adv_gen < 0 ? 0 : t.n;
}

int hk_poca_stats(hk_handle h, int trainer, float* out)
{
    int rc = poca_field_check(h, trainer, 0, "hk_poca_stats");
    if (rc) return rc;
    if (!out) return fail(h, HK_ERR_INVALID, "hk_poca_stats: NULL out");
    const auto& t = h->train->ppo[trainer];
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
    if (pool < 0 || pool >= h->train->n_pools) return fail(h, HK_ERR_INVALID, f + ": bad pool index");
    const auto& pl = h->train->pool[pool];
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
    if (h->train->n_pools >= HK_MAX_POOLS) return fail(h, HK_ERR_INVALID, f + "HK_MAX_POOLS pools already exist");
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
    h->train->pool[h->train->n_pools] = pl;
    return h->train->n_pools++;
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
    if (pool < 0 || pool >= h->train->n_pools) return fail(h, HK_ERR_INVALID, "hk_policy_pool_count: bad pool index");
    return (int)h->train->pool[pool].count;
}

int hk_policy_pool_save(hk_handle h, int pool, int slot, int policy)
{
    HK_NEED_ENV(h);
    if (policy == -1) policy = -2;
    int rc = pool_check(h, "hk_policy_pool_save", pool, slot, policy);
    if (rc) return rc;
    auto& pl = h->train->pool[pool];
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
    const auto& pl = h->train->pool[pool];
    if (!((pl.filled >> slot) & 1ull)) return fail(h, HK_ERR_INVALID, "hk_policy_pool_load: the slot has never been written (hk_policy_pool_save / hk_policy_pool_put)");
    if ((rc = ppo_refuse_open(h, "hk_policy_pool_load"))) return rc;
    for (int i = 0; i < h->train->n_ppo; i++)
        if (h->train->ppo[i].policy == policy)
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
    if (pd.wlbf) HK_HIP(h, hk::policy_lstm_bf16_refresh(pd.q, pd.lq, pd.lbq, h->stream));      // (a recurrent pool into a bf16 policy with memory: the cell's)
    return HK_OK;
}

int hk_policy_pool_put(hk_handle h, int pool, int slot, const float* flat)
{
    HK_NEED_ENV(h);
    int rc = pool_check(h, "hk_policy_pool_put", pool, slot, -1);
    if (rc) return rc;
    if (!flat) return fail(h, HK_ERR_INVALID, "hk_policy_pool_put: NULL pointer");
    auto& pl = h->train->pool[pool];
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
    const auto& pl = h->train->pool[pool];
    if (!((pl.filled >> slot) & 1ull)) return fail(h, HK_ERR_INVALID, "hk_policy_pool_get: the slot has never been written");
    HK_HIP(h, hipMemcpyAsync(flat, pool_slot(pl, slot), pl.count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HK_HIP(h, hipStreamSynchronize(h->stream));
    return HK_OK;
}

}  // extern "C"

hk::TrainState* hk::train_create() { return new (std::nothrow) TrainState(); }

void hk::train_destroy(hk_context* h)
{
    if (!h->train) return;
    for (auto& t : h->train->ppo) ppo_release(t);
    for (auto& pl : h->train->pool) if (pl.buf) (void)hipFree(pl.buf);
    delete h->train;
    h->train = nullptr;
}
