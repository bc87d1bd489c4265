// Host check of the plain arithmetic of recurrent training (csrc/hk_lstm_train.h; hk.h "PPO trainer" RECURRENT): a stand-alone program that runs
// the SAME hk_lstm_cell_back and hk_seq_row the kernels compile (one HK_HD definition each).  Built and run by tests/test_ppo_lstm_cpu.py:
//   g++ -O2 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//   ppo_lstm_host_check      prints "name value" lines:
//     cell_back_max_err  hk_lstm_cell_back (fp32) on N random units against the float64 gradient of L = wh h' + wc c' through the cell's formula
//                            (sigma and tanh of libm), obtained by central differences in float64; absolute, over |wh| + |wc|
//     cell_forward_max_err   hk_lstm_cell (fp32) against the same float64 formula, the check of the reference itself
//     seq_mismatches         hk_seq_row against a brute-force enumeration of (t, e, j) over several (R, L, E, S), out-of-range ids included
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>
#include "../hierarchicalkarting_amd/csrc/hk_lstm_train.h"

static double sig(double z) { return 1.0 / (1.0 + std::exp(-z)); }

// L = wh h' + wc c' of the pre-activations z[4] and c
static double cell_loss(const double* z, double c, double wh, double wc)
{
    const double i = sig(z[0]), f = sig(z[1]), g = std::tanh(z[2]), o = sig(z[3]);
    const double cn = f * c + i * g;
    return wh * (o * std::tanh(cn)) + wc * cn;
}

static uint32_t rng_state = 0x1234567u;
static double urand(double lo, double hi)
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return lo + (hi - lo) * ((rng_state >> 8) / 16777216.0);
}

int main()
{
    double worst_back = 0.0, worst_fwd = 0.0;
    for (int n = 0; n < 20000; n++) {
        double z[4];
        for (double& x : z) x = urand(-4.0, 4.0);
        const double c = urand(-2.0, 2.0), wh = (float)urand(-1.0, 1.0), wc = (float)urand(-1.0, 1.0);          // (fp32 values: both sides see the same)
        const float zf[4] = {(float)z[0], (float)z[1], (float)z[2], (float)z[3]};
        const float cf = (float)c;
        for (int q = 0; q < 4; q++) z[q] = zf[q];          // the reference sees the fp32 inputs
        const double cd = cf;
        float hn, cn;
        hk_lstm_cell(zf[0], zf[1], zf[2], zf[3], cf, &hn, &cn);
        const double i = sig(z[0]), f = sig(z[1]), g = std::tanh(z[2]), o = sig(z[3]);
        const double cnd = f * cd + i * g, hnd = o * std::tanh(cnd);
        worst_fwd = std::fmax(worst_fwd, std::fmax(std::fabs(hn - hnd), std::fabs(cn - cnd)));
        // float64 central differences of L with respect to z[0..3] and c
        double ref[5];
        const double hstep = 1e-6;
        for (int q = 0; q < 5; q++) {
            double zp[4] = {z[0], z[1], z[2], z[3]}, zm[4] = {z[0], z[1], z[2], z[3]}, cp = cd, cm = cd;
            if (q < 4) { zp[q] += hstep; zm[q] -= hstep; } else { cp += hstep; cm -= hstep; }
            ref[q] = (cell_loss(zp, cp, wh, wc) - cell_loss(zm, cm, wh, wc)) / (2.0 * hstep);
        }
        float dz[4], dcp;
        hk_lstm_cell_back((float)wh, (float)wc, hk_sigmoidf(zf[0]), hk_sigmoidf(zf[1]), hk_tanhf_fast(zf[2]), hk_sigmoidf(zf[3]), cn, cf, dz, &dcp);
        const double scale = std::fabs(wh) + std::fabs(wc) + 1e-30;          // every output is dh or dc (<= |wh| + |wc|) times factors in [0, 1]
        const float got[5] = {dz[0], dz[1], dz[2], dz[3], dcp};
        for (int q = 0; q < 5; q++) worst_back = std::fmax(worst_back, std::fabs(got[q] - ref[q]) / scale);
    }
    std::printf("cell_back_max_err %.6g\n", worst_back);
    std::printf("cell_forward_max_err %.6g\n", worst_fwd);
    long mismatches = 0;
    const int shapes[][4] = {{12, 4, 3, 2}, {11, 4, 3, 2}, {1, 4, 2, 1}, {9, 1, 2, 2}, {5, 64, 1, 3}, {11, 4, 70, 2}};
    for (const auto& sh : shapes) {
        const int R = sh[0], L = sh[1], E = sh[2], S = sh[3], ES = E * S, nseq = (R + L - 1) / L * ES;
        std::map<std::pair<int, int>, int> brute;          // (sid, tau) -> row id
        for (int t = 0; t < R; t++)
            for (int e = 0; e < E; e++)
                for (int j = 0; j < S; j++) brute[{((t / L) * E + e) * S + j, t % L}] = (t * E + e) * S + j;
        for (int sid = -3; sid < nseq + 3; sid++)
            for (int tau = 0; tau < L; tau++) {
                int t = -1;
                const int rid = hk_seq_row(sid, tau, L, R, ES, nseq, &t);
                const auto it = brute.find({sid, tau});
                const int want = it == brute.end() ? -1 : it->second;
                if (rid != want || (rid >= 0 && t != rid / ES)) mismatches++;
            }
    }
    std::printf("seq_mismatches %ld\n", mismatches);
    return 0;
}
