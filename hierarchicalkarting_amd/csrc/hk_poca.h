// hk_poca.h — device side of the POCA trainer (contract in include/hk.h "POCA", host side in hk_train.hip).
// A POCA trainer is a PPO trainer whose critic is a centralised attention critic over the S agents of a group (the policy's slots in one env).
// Per minibatch of mg groups (m = mg S agent rows, E2 = 2 m entities, NS = (S + 1) mg sequences, SR = NS S sequence rows):
//   poca_rows_kernel        group ids -> the agent row ids ppo_gather_kernel reads (a bootstrap group -> the bootstrap rows; any other id -> -1)
//   poca_actfeat_kernel     XA [m][in_dim + 1 + n_branch] = [x ; RAW ; onehot(BRANCH)]: the W_act product runs over this gathered row
//   ppo_gemm_kernel<EPI>    every linear product (hk_ppo.h): the two embeddings and the encoder (EPI 1 / 2), q, k, v, out (EPI 0, bias seed),
//                           the weight gradients (split-K of PPO_KCH rows, ppo_combine_kernel), the biases by ppo_colsum_kernel
//   poca_ln_kernel<RES>     LayerNorm of a row, one wave per row, the lanes over H; RES: of (row + the entity's normalised embedding), the
//                           residual of the attention block.  Keeps the row's mean and 1 / sigma.
//   poca_attn_fwd / bwd     the attention core, one wave per sequence: 16 lanes per head, a head's dot products reduced across its 16 lanes
//                           (xor butterflies: every lane of the head ends with the same bits), the S x S scores and weights in registers
//   poca_pool_kernel, poca_out_bwd_kernel     the mean over a sequence's S positions; its backward fused with the out-LayerNorm's
//   poca_entsum_kernel      the sequences' gradients of q, k, v and the residual summed into their entity, in sequence order
//   poca_ent_bwd_kernel     the entity LayerNorm's backward times swish' of the embedding
//   poca_value_kernel, poca_scatter_kernel    the one head over the NS sequences; V / B to the rows' buffers or the minibatch's
//   poca_loss_kernel        runs after ppo_loss_kernel (which is given the row's group value as a 1-wide "activation": its code is untouched):
//                           the baseline's clipped loss, and dL / d(output) of every sequence
//   poca_stats_kernel       L_b, and the skipped count in groups
//   poca_lambda_kernel      one lane per (e, j): the team reward and the lambda-return, backwards over t
// No float atomics; every sum has a fixed order.
#pragma once
#include "hk_ppo.h"

namespace hk {

constexpr int POCA_HEADS = 4, POCA_MAXS = 4;

// flat layout of the POCA critic, in the order of hk_poca_critic_desc
struct PocaNet {
    int in_dim = 0, n_act = 0, hidden = 0, n_layers = 0, n_branch = 0;
    size_t oWobs = 0, obobs = 0, oWact = 0, obact = 0, oWq = 0, obq = 0, oWk = 0, obk = 0, oWv = 0, obv = 0, oWout = 0, obout = 0;
    size_t oW[HK_POLICY_MAX_LAYERS] = {}, ob[HK_POLICY_MAX_LAYERS] = {};
    size_t owval = 0, obval = 0, count = 0;
    void layout(int in, int nb, int H, int L, size_t base)
    {
        in_dim = in; n_branch = nb; n_act = in + 1 + nb; hidden = H; n_layers = L;
        size_t o = base;
        oWobs = o; o += (size_t)H * in; obobs = o; o += H;
        oWact = o; o += (size_t)H * n_act; obact = o; o += H;
        oWq = o; o += (size_t)H * H; obq = o; o += H;
        oWk = o; o += (size_t)H * H; obk = o; o += H;
        oWv = o; o += (size_t)H * H; obv = o; o += H;
        oWout = o; o += (size_t)H * H; obout = o; o += H;
        for (int l = 0; l < L; l++) { oW[l] = o; o += (size_t)H * H; ob[l] = o; o += H; }
        owval = o; o += H; obval = o; o += 1;
        count = o - base;
    }
};

// Sequence q of a group (q = 0: the value sequence, q = 1 + a: agent a's baseline sequence), position p -> the entity's row in the [2 m]
// entity buffers: the obs entity of (group i, agent j) is row i S + j, its act entity row m + i S + j.
__device__ __forceinline__ int poca_entity(int i, int q, int p, int S, int m)
{
    if (q == 0) return i * S + p;
    const int a = q - 1;
    if (p == 0) return i * S + a;
    const int k = (p - 1 < a) ? p - 1 : p;
    return m + i * S + k;
}

__device__ __forceinline__ float poca_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float poca_head_sum(float v)          // over the 16 lanes of a head
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// gids [mg] -> rid [mg S]; G = R E groups, boot: a group id in [G, G + E) is the bootstrap group of env id - G
__global__ __launch_bounds__(256) void poca_rows_kernel(const int* gids, int mg, int S, int G, int E, int boot, int* rid)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= mg * S) return;
    const int g = gids[x / S], j = x % S;
    int r = -1;
    if (g >= 0 && g < G) r = g * S + j;
    else if (boot && g >= G && g < G + E) r = G * S + (g - G) * S + j;
    rid[x] = r;
}

__global__ __launch_bounds__(256) void poca_actfeat_kernel(PpoRows P, const int* rid, int m, const float* X0, float* XA, int nb)
{
    const int na = P.in_dim + 1 + nb;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)m * na) return;
    const int i = (int)(idx / na), k = (int)(idx % na);
    if (k < P.in_dim) { XA[idx] = X0[(size_t)i * P.in_dim + k]; return; }
    const int id = rid[i], n = P.R * P.E * P.S;
    float v = 0.0f;
    if (id >= 0 && id < n) {          // (a bootstrap row has no action: its baseline is never read)
        const int t = id / (P.E * P.S), e = (id / P.S) % P.E, j = id % P.S;
        const size_t ea = ((size_t)t * P.E + e) * P.A + P.slots[j];
        v = k == P.in_dim ? P.raw[ea] : (P.branch[ea] == k - P.in_dim - 1 ? 1.0f : 0.0f);
    }
    XA[idx] = v;
}

// Y[row] = LN(U[row] (+ Nent[entity of the sequence row])), stat[row] = (mean, 1 / sqrt(var + 1e-5)); population variance, no affine; H <= 256
template <bool RES>
__global__ __launch_bounds__(256) void poca_ln_kernel(const float* __restrict__ U, const float* __restrict__ Nent, int rows, int H, int S, int m,
                                                      float* __restrict__ Y, float2* __restrict__ stat)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    int ent = 0;
    if (RES) { const int seq = row / S, p = row % S; ent = poca_entity(seq / (S + 1), seq % (S + 1), p, S, m); }
    float u[4], s = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int h = lane + 64 * c;
        u[c] = 0.0f;
        if (h < H) {
            u[c] = U[(size_t)row * H + h];
            if (RES) u[c] += Nent[(size_t)ent * H + h];
            s += u[c];
        }
    }
    const float mean = poca_wave_sum(s) / (float)H;
    float v = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; c++) if (lane + 64 * c < H) { const float d = u[c] - mean; v += d * d; }
    const float rstd = 1.0f / sqrtf(poca_wave_sum(v) / (float)H + 1e-5f);
#pragma unroll
    for (int c = 0; c < 4; c++) if (lane + 64 * c < H) Y[(size_t)row * H + lane + 64 * c] = (u[c] - mean) * rstd;
    if (lane == 0) stat[row] = make_float2(mean, rstd);
}

// dX[row] = rstd (dy - mean(dy) - y mean(dy y)) for one row held as up to 4 elements per lane
__device__ __forceinline__ void poca_ln_back(float (&dy)[4], const float (&y)[4], float rstd, int lane, int H)
{
    float a = 0.0f, b = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; c++) if (lane + 64 * c < H) { a += dy[c]; b += dy[c] * y[c]; }
    const float m1 = poca_wave_sum(a) / (float)H, m2 = poca_wave_sum(b) / (float)H;
#pragma unroll
    for (int c = 0; c < 4; c++) dy[c] = rstd * (dy[c] - m1 - y[c] * m2);
}

// the attention core of one sequence: alpha = softmax_r(<q_s^h, k_r^h> / sqrt(H)), c_s^h = sum_r alpha_sr v_r^h.
// lane = 16 head + sub; sub owns the head's columns sub, sub + 16, ... (head width H / 4 <= 64)
struct PocaSeq { int ent[POCA_MAXS]; };
__device__ __forceinline__ PocaSeq poca_seq(int seq, int S, int m)
{
    PocaSeq e;
#pragma unroll
    for (int p = 0; p < POCA_MAXS; p++) e.ent[p] = p < S ? poca_entity(seq / (S + 1), seq % (S + 1), p, S, m) : 0;
    return e;
}

__global__ __launch_bounds__(256) void poca_attn_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, int nseq, int S,
                                                            int m, int H, float* __restrict__ Cout, float* __restrict__ alpha)
{
    const int seq = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (seq >= nseq) return;
    const int head = lane >> 4, sub = lane & 15, dw = H / POCA_HEADS;
    const PocaSeq e = poca_seq(seq, S, m);
    float q[POCA_MAXS][4], k[POCA_MAXS][4], v[POCA_MAXS][4];
#pragma unroll
    for (int p = 0; p < POCA_MAXS; p++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int d = sub + 16 * c;
            const bool ok = p < S && d < dw;
            const size_t o = (size_t)e.ent[p] * H + head * dw + d;
            q[p][c] = ok ? Q[o] : 0.0f; k[p][c] = ok ? K[o] : 0.0f; v[p][c] = ok ? V[o] : 0.0f;
        }
    const float scale = sqrtf((float)H);
    float al[POCA_MAXS][POCA_MAXS];
#pragma unroll
    for (int s = 0; s < POCA_MAXS; s++) {
        float sc[POCA_MAXS], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < POCA_MAXS; r++) {
            float d = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; c++) d += q[s][c] * k[r][c];
            sc[r] = poca_head_sum(d) / scale;
            if (r < S && sc[r] > mx) mx = sc[r];
        }
        float tot = 0.0f;
#pragma unroll
        for (int r = 0; r < POCA_MAXS; r++) { sc[r] = r < S ? expf(sc[r] - mx) : 0.0f; tot += sc[r]; }
#pragma unroll
        for (int r = 0; r < POCA_MAXS; r++) al[s][r] = sc[r] / tot;
    }
#pragma unroll
    for (int s = 0; s < POCA_MAXS; s++) {
        if (s >= S) continue;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int d = sub + 16 * c;
            if (d >= dw) continue;
            float o = 0.0f;
#pragma unroll
            for (int r = 0; r < POCA_MAXS; r++) o += al[s][r] * v[r][c];
            Cout[((size_t)seq * S + s) * H + head * dw + d] = o;
        }
        if (sub == 0) {
#pragma unroll
            for (int r = 0; r < POCA_MAXS; r++) alpha[(((size_t)seq * POCA_HEADS + head) * POCA_MAXS + s) * POCA_MAXS + r] = al[s][r];
        }
    }
}

// backward of the core: per sequence row dq, dk, dv [SR][H] from dC [SR][H] and the weights the forward kept
__global__ __launch_bounds__(256) void poca_attn_bwd_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                            const float* __restrict__ alpha, const float* __restrict__ dC, int nseq, int S, int m, int H,
                                                            float* __restrict__ dQs, float* __restrict__ dKs, float* __restrict__ dVs)
{
    const int seq = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (seq >= nseq) return;
    const int head = lane >> 4, sub = lane & 15, dw = H / POCA_HEADS;
    const PocaSeq e = poca_seq(seq, S, m);
    float q[POCA_MAXS][4], k[POCA_MAXS][4], v[POCA_MAXS][4], dc[POCA_MAXS][4];
#pragma unroll
    for (int p = 0; p < POCA_MAXS; p++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int d = sub + 16 * c;
            const bool ok = p < S && d < dw;
            const size_t o = (size_t)e.ent[p] * H + head * dw + d;
            q[p][c] = ok ? Q[o] : 0.0f; k[p][c] = ok ? K[o] : 0.0f; v[p][c] = ok ? V[o] : 0.0f;
            dc[p][c] = ok ? dC[((size_t)seq * S + p) * H + head * dw + d] : 0.0f;
        }
    const float scale = sqrtf((float)H);
    float al[POCA_MAXS][POCA_MAXS], ds[POCA_MAXS][POCA_MAXS];
#pragma unroll
    for (int s = 0; s < POCA_MAXS; s++) {
        float da[POCA_MAXS], dot = 0.0f;
#pragma unroll
        for (int r = 0; r < POCA_MAXS; r++) {
            al[s][r] = (s < S && r < S) ? alpha[(((size_t)seq * POCA_HEADS + head) * POCA_MAXS + s) * POCA_MAXS + r] : 0.0f;
            float d = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; c++) d += dc[s][c] * v[r][c];
            da[r] = poca_head_sum(d);
            dot += al[s][r] * da[r];
        }
#pragma unroll
        for (int r = 0; r < POCA_MAXS; r++) ds[s][r] = al[s][r] * (da[r] - dot) / scale;
    }
#pragma unroll
    for (int p = 0; p < POCA_MAXS; p++) {
        if (p >= S) continue;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int d = sub + 16 * c;
            if (d >= dw) continue;
            float gq = 0.0f, gk = 0.0f, gv = 0.0f;
#pragma unroll
            for (int r = 0; r < POCA_MAXS; r++) {
                gq += ds[p][r] * k[r][c];
                gk += ds[r][p] * q[r][c];
                gv += al[r][p] * dc[r][c];
            }
            const size_t o = ((size_t)seq * S + p) * H + head * dw + d;
            dQs[o] = gq; dKs[o] = gk; dVs[o] = gv;
        }
    }
}

// Zp[seq][h] = (sum_p O[seq][p][h], p ascending) / S
__global__ __launch_bounds__(256) void poca_pool_kernel(const float* __restrict__ O, int nseq, int S, int H, float* __restrict__ Zp)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)nseq * H) return;
    const size_t seq = idx / H, h = idx % H;
    float s = O[(seq * S) * H + h];
    for (int p = 1; p < S; p++) s += O[(seq * S + p) * H + h];
    Zp[idx] = s / (float)S;
}

// dPre[row] = the out-LayerNorm's backward of dO[row] = dZp[seq] / S; O is the LayerNorm's output, stat its (mean, 1 / sigma)
__global__ __launch_bounds__(256) void poca_out_bwd_kernel(const float* __restrict__ dZp, const float* __restrict__ O, const float2* __restrict__ stat, int rows,
                                                           int S, int H, float* __restrict__ dPre)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int seq = row / S;
    float dy[4], y[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int h = lane + 64 * c;
        const bool ok = h < H;
        dy[c] = ok ? dZp[(size_t)seq * H + h] / (float)S : 0.0f;
        y[c] = ok ? O[(size_t)row * H + h] : 0.0f;
    }
    poca_ln_back(dy, y, stat[row].y, lane, H);
#pragma unroll
    for (int c = 0; c < 4; c++) if (lane + 64 * c < H) dPre[(size_t)row * H + lane + 64 * c] = dy[c];
}

// an entity's gradients: the sequence rows it stands in, summed in sequence order.  obs (i, j): (q 0, p j), (q 1 + j, p 0);
// act (i, k): q = 1 + a for a != k ascending, at p = k < a ? k + 1 : k
__global__ __launch_bounds__(256) void poca_entsum_kernel(const float* __restrict__ dQs, const float* __restrict__ dKs, const float* __restrict__ dVs,
                                                          const float* __restrict__ dPre, int S, int m, int H, float* __restrict__ dQ, float* __restrict__ dK,
                                                          float* __restrict__ dV, float* __restrict__ dR)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)2 * m * H) return;
    const int ent = (int)(idx / H), h = (int)(idx % H);
    const bool act = ent >= m;
    const int x = act ? ent - m : ent, i = x / S, j = x % S;
    float a = 0.0f, b = 0.0f, c = 0.0f, d = 0.0f;
    auto add = [&](int q, int p) {
        const size_t o = (((size_t)i * (S + 1) + q) * S + p) * H + h;
        a += dQs[o]; b += dKs[o]; c += dVs[o]; d += dPre[o];
    };
    if (!act) { add(0, j); add(1 + j, 0); }
    else for (int aa = 0; aa < S; aa++) if (aa != j) add(1 + aa, j < aa ? j + 1 : j);
    dQ[idx] = a; dK[idx] = b; dV[idx] = c; dR[idx] = d;
}

// dZ[ent] = LNback(dR + dNq + dNk + dNv) * swish'(Z[ent]); N is the entity LayerNorm's output
__global__ __launch_bounds__(256) void poca_ent_bwd_kernel(const float* __restrict__ dR, const float* __restrict__ dNq, const float* __restrict__ dNk,
                                                           const float* __restrict__ dNv, const float* __restrict__ N, const float2* __restrict__ stat,
                                                           const float* __restrict__ Z, int rows, int H, float* __restrict__ dZ)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float dy[4], y[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const size_t o = (size_t)row * H + lane + 64 * c;
        const bool ok = lane + 64 * c < H;
        dy[c] = ok ? ((dR[o] + dNq[o]) + dNk[o]) + dNv[o] : 0.0f;
        y[c] = ok ? N[o] : 0.0f;
    }
    poca_ln_back(dy, y, stat[row].y, lane, H);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        if (lane + 64 * c >= H) continue;
        const size_t o = (size_t)row * H + lane + 64 * c;
        const float zz = Z[o];
        const float sg = 1.0f / (1.0f + expf(-zz));
        dZ[o] = dy[c] * (sg + zz * sg * (1.0f - sg));
    }
}

// out[seq] = <w_val, Y[seq]> + b_val: the heads' fmaf chain (pm_head)
__global__ __launch_bounds__(256) void poca_value_kernel(const float* Y, int nseq, int H, const float* w_val, const float* b_val, float* out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nseq) out[i] = pm_head(Y + (size_t)i * H, 1, w_val, b_val[0], H);
}

// agent row x = (group i, agent j) of the minibatch: V = out[i (S + 1)], B = out[i (S + 1) + 1 + j] -> whichever targets are given.
// rows: v_old / b_old [n] at rid (v_boot [E S] for a bootstrap row);  minibatch: vrow / brow [m], mbv [mg]
__global__ __launch_bounds__(256) void poca_scatter_kernel(const float* out, const int* rid, int m, int S, int n, int nboot, float* v_old, float* b_old, float* v_boot,
                                                           float* vrow, float* brow, float* mbv)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= m) return;
    const int i = x / S, j = x % S;
    const float v = out[i * (S + 1)], b = out[i * (S + 1) + 1 + j];
    if (vrow) { vrow[x] = v; brow[x] = b; if (j == 0) mbv[i] = v; }
    if (v_old) {
        const int id = rid[x];
        if (id >= 0 && id < n) { v_old[id] = v; b_old[id] = b; }
        else if (id >= n && id < n + nboot) v_boot[id - n] = v;
    }
}

// One thread per group, after ppo_loss_kernel (dv [m]: its 0.5 / m_valid dL_v / dv per row).  The baseline's clipped loss (torch.max: a tie
// splits; the clamp passes inside [-eps, eps]) with weight 0.25 / m_valid, its row stat, and dL / d(output) of the group's S + 1 sequences:
// the value sequence collects its S rows' dv in row order.
__global__ __launch_bounds__(256) void poca_loss_kernel(const float* brow, const int* rid, const int* valid, const int* n_valid, const float* b_old,
                                                        const float* ret, const float* dv, int mg, int S, int n, float eps, float* dout, double* rowstat_b)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mg) return;
    const float inv = 1.0f / (float)n_valid[0];
    float dvs = 0.0f;
    for (int j = 0; j < S; j++) {
        const int x = i * S + j, id = rid[x];
        float g = 0.0f;
        double st = 0.0;
        if (valid[x] && id >= 0 && id < n) {
            const float b = brow[x], bo = b_old[id], R = ret[id];
            const float dbb = b - bo;
            const float dc = dbb < -eps ? -eps : (dbb > eps ? eps : dbb);
            const float a1 = R - b, b1 = R - bo - dc;
            const float f1 = a1 * a1, f2 = b1 * b1;
            const float g1 = -2.0f * a1, g2 = (dbb >= -eps && dbb <= eps) ? -2.0f * b1 : 0.0f;
            const float gb = f1 > f2 ? g1 : (f1 < f2 ? g2 : 0.5f * (g1 + g2));
            g = 0.25f * inv * gb;
            st = f1 > f2 ? f1 : f2;
            dvs += dv[x];
        }
        dout[i * (S + 1) + 1 + j] = g;
        rowstat_b[x] = st;
    }
    dout[i * (S + 1)] = dvs;
}

// pstats[0] = L_b = sum rowstat_b / valid rows (one workgroup, fixed order), pstats[1] = 0; the skipped count of stats / acc from rows to groups;
// pacc != nullptr: pacc[0] += L_b, pacc[1] += 1
__global__ __launch_bounds__(256) void poca_stats_kernel(const double* rowstat_b, int m, int S, const int* n_valid, float* stats, double* acc, float* pstats, double* pacc)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < m; i += 256) s += rowstat_b[i];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
    if (tid == 0) {
        const int nv = n_valid[0];
        const double lb = red[0] / (double)(nv > 0 ? nv : 1);
        pstats[0] = (float)lb; pstats[1] = 0.0f;
        const double rows = (double)stats[5], groups = rows / (double)S;
        stats[5] = (float)groups;
        if (acc) acc[5] += groups - rows;
        if (pacc) { pacc[0] += lb; pacc[1] += 1.0; }
    }
}

// One lane per (e, j), t from R - 1 down (hk.h "POCA"): rho = (sum_k r_k, k ascending) + g_j;  G_t = rho + gamma (1 - d) ((1 - lambda) V_{t+1} + lambda G_{t+1});
// G_R = V_R = the bootstrap value.  RET = G, ADV = G - B.  v_old / v_boot hold the group's value once per agent.
__global__ __launch_bounds__(256) void poca_lambda_kernel(PpoRows P, const float* group_reward, const float* term_group_reward, const float* v_old, const float* b_old,
                                                          const float* v_boot, float gamma, float lambd, float* team, float* adv, float* ret)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P.E * P.S) return;
    const int e = p / P.S, j = p % P.S;
    float vnext = v_boot[p], gnext = v_boot[p];
    for (int t = P.R - 1; t >= 0; t--) {
        const size_t g = (size_t)t * P.E + e, r = g * P.S + j;
        const int d = P.done[g] != 0;
        const float* rw = d ? P.term_reward : P.reward;
        float rho = rw[g * P.A + P.slots[0]];
        for (int k = 1; k < P.S; k++) rho = rho + rw[g * P.A + P.slots[k]];
        rho = rho + (d ? term_group_reward : group_reward)[g * P.A + P.slots[j]];
        const float nd = d ? 0.0f : 1.0f;
        const float G = rho + gamma * nd * ((1.0f - lambd) * vnext + lambd * gnext);
        team[r] = rho; ret[r] = G; adv[r] = G - b_old[r];
        vnext = v_old[r]; gnext = G;
    }
}

}  // namespace hk
