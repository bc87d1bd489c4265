// hk_lstm_train.h — the two pieces of recurrent training (hk_ppo_lstm.h; hk.h "PPO trainer" RECURRENT) that are plain arithmetic:
// the cell's backward on one unit and the sequence-id -> row-id rule.  Plain C (HK_HD), ONE definition each, shared by ppo_lstm_back_kernel /
// ppo_lstm_expand_kernel and by the host build of tests/ppo_lstm_host_check.cpp, which checks them against float64 finite differences of
// hk_lstm_cell's formula and against a brute-force enumeration.
#pragma once
#include "hk_policy_lstm.h"

/* The cell backward of one unit.  dh: dL/dh' (the heads' delta plus the recurrent delta), dc_in: dL/dc' carried from the step after; gi gf gg go:
 * the stored gate outputs i f g~ o; c_new: the stored c'; c_prev: the c the row read (after the reset).
 * sigma' = s (1 - s), tanh' = 1 - t^2.  -> dz[4]: dL/d(pre-activation) of i f g o;  *dc_prev: dL/dc, what the step before adds to its dc. */
HK_HD void hk_lstm_cell_back(float dh, float dc_in, float gi, float gf, float gg, float go, float c_new, float c_prev, float* dz, float* dc_prev)
{
    const float tc = hk_tanhf_fast(c_new);
    const float dc = dc_in + dh * go * (1.0f - tc * tc);
    dz[0] = dc * gg * (gi * (1.0f - gi));
    dz[1] = dc * c_prev * (gf * (1.0f - gf));
    dz[2] = dc * gi * (1.0f - gg * gg);
    dz[3] = dh * tc * (go * (1.0f - go));
    *dc_prev = dc * gf;
}

/* Sequence id s = (k E + e) S + j, ES = E S, n_seq = ceil(R / L) ES: the row id (t E + e) S + j of its step tau, t = k L + tau; -1 where the row is
 * dead (t >= R) or the id lies outside [0, n_seq).  *t_out (when not NULL and the row is live): t. */
HK_HD int hk_seq_row(int sid, int tau, int L, int R, int ES, int n_seq, int* t_out)
{
    if (sid < 0 || sid >= n_seq) return -1;
    const int k = sid / ES, rem = sid - k * ES, t = k * L + tau;
    if (t >= R) return -1;
    if (t_out) *t_out = t;
    return t * ES + rem;
}
