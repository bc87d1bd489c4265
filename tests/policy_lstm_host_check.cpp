// Host twin of policy_lstm_kernel (csrc/hk_policy_lstm.h; hk.h "RECURRENT ACTORS"): a stand-alone program that evaluates a recurrent actor on the
// CPU with the SAME hk_sigmoidf / hk_tanhf_fast / hk_lstm_cell the kernel compiles (one HK_HD definition each) and the contract's k-ascending
// fmaf chains for the trunk, the gate pre-activations and the heads.  It is the bit reference of tests/test_policy_lstm_gpu.py and is compared
// with an independent float64 restatement (tests/policy_lstm_restate.py) in tests/test_policy_lstm_cpu.py.  Built by tests/policy_lstm_twin.py:
//   g++ -O2 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -pthread
//
//   policy_lstm_host_check CASE OUT     one step of every row of CASE -> OUT
//     CASE: int32 {magic 0x4C53544D, in_dim, hidden, n_layers, n_branch, normalize, m, rows}, then float32:
//           mean[in_dim], std[in_dim] (when normalize); per layer W[hidden][k], b[hidden]; W_ih[4m][hidden], W_hh[4m][m], b_ih[4m], b_hh[4m];
//           W_mu[m], b_mu[1], W_branch[n_branch][m], b_branch[n_branch]; obs[rows][in_dim] (stacked, oldest first); mem[rows][2m] = [h | c]
//     OUT:  float32 mu[rows], logits[rows][n_branch], mem[rows][2m]
//   policy_lstm_host_check --sweep      hk_sigmoidf and hk_tanhf_fast over every finite fp32 input against libm in double: prints
//                                       "sigmoid_max_abs_err E", "tanh_max_abs_err E" and the values at +-Inf and NaN
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include "../hierarchicalkarting_amd/csrc/hk_policy_lstm.h"

static float chain(float s, const float* a, const float* w, int n)
{
    for (int k = 0; k < n; k++) s = __builtin_fmaf(a[k], w[k], s);
    return s;
}

static int run_case(const char* in_path, const char* out_path)
{
    FILE* f = std::fopen(in_path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", in_path); return 2; }
    int32_t hd[8];
    if (std::fread(hd, 4, 8, f) != 8 || hd[0] != 0x4C53544D) { std::fprintf(stderr, "bad header\n"); return 2; }
    const int K0 = hd[1], H = hd[2], NL = hd[3], NB = hd[4], norm = hd[5], m = hd[6], rows = hd[7];
    auto take = [&](size_t n) {
        std::vector<float> v(n);
        if (n && std::fread(v.data(), 4, n, f) != n) { std::fprintf(stderr, "short case file\n"); std::exit(2); }
        return v;
    };
    std::vector<float> mean, sdev;
    if (norm) { mean = take(K0); sdev = take(K0); }
    std::vector<std::vector<float>> W(NL), b(NL);
    for (int l = 0; l < NL; l++) { W[l] = take((size_t)H * (l == 0 ? K0 : H)); b[l] = take(H); }
    const std::vector<float> W_ih = take((size_t)4 * m * H), W_hh = take((size_t)4 * m * m), b_ih = take(4 * m), b_hh = take(4 * m);
    const std::vector<float> W_mu = take(m), b_mu = take(1), W_br = take((size_t)NB * m), b_br = take(NB);
    const std::vector<float> obs = take((size_t)rows * K0);
    std::vector<float> mem = take((size_t)rows * 2 * m);
    std::fclose(f);

    std::vector<float> bsum(4 * m), mu(rows), lg((size_t)rows * NB);
    for (int k = 0; k < 4 * m; k++) bsum[k] = b_ih[k] + b_hh[k];
    std::vector<float> x(K0 > H ? K0 : H), y(H), hn(m), cn(m), z(4);
    for (int r = 0; r < rows; r++) {
        for (int k = 0; k < K0; k++) {
            float v = obs[(size_t)r * K0 + k];
            if (norm) { v = (v - mean[k]) / sdev[k]; v = v < -5.0f ? -5.0f : (v > 5.0f ? 5.0f : v); }
            x[k] = v;
        }
        for (int l = 0; l < NL; l++) {
            const int K = l == 0 ? K0 : H;
            for (int j = 0; j < H; j++) y[j] = hk_swishf(chain(b[l][j], x.data(), &W[l][(size_t)j * K], K));
            for (int j = 0; j < H; j++) x[j] = y[j];
        }
        float* h = &mem[(size_t)r * 2 * m];
        float* c = h + m;
        for (int j = 0; j < m; j++) {
            for (int g = 0; g < 4; g++) {
                const int col = g * m + j;
                z[g] = chain(chain(bsum[col], x.data(), &W_ih[(size_t)col * H], H), h, &W_hh[(size_t)col * m], m);
            }
            hk_lstm_cell(z[0], z[1], z[2], z[3], c[j], &hn[j], &cn[j]);
        }
        for (int j = 0; j < m; j++) { h[j] = hn[j]; c[j] = cn[j]; }
        mu[r] = chain(b_mu[0], h, W_mu.data(), m);
        for (int q = 0; q < NB; q++) lg[(size_t)r * NB + q] = chain(b_br[q], h, &W_br[(size_t)q * m], m);
    }
    FILE* o = std::fopen(out_path, "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", out_path); return 2; }
    std::fwrite(mu.data(), 4, mu.size(), o);
    std::fwrite(lg.data(), 4, lg.size(), o);
    std::fwrite(mem.data(), 4, mem.size(), o);
    std::fclose(o);
    return 0;
}

static float from_bits(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }

static int sweep()
{
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    std::vector<double> es(nt, 0.0), et(nt, 0.0);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t]() {
            double ms = 0.0, mt = 0.0;
            // every bit pattern with a finite value: exponent field below 0xFF, both signs
            for (uint64_t u = t; u < 0x100000000ull; u += nt) {
                if ((u & 0x7F800000u) == 0x7F800000u) continue;
                const float x = from_bits((uint32_t)u);
                const double ds = std::fabs((double)hk_sigmoidf(x) - 1.0 / (1.0 + std::exp(-(double)x)));
                const double dt = std::fabs((double)hk_tanhf_fast(x) - std::tanh((double)x));
                if (!(ds <= ms)) ms = ds;
                if (!(dt <= mt)) mt = dt;
            }
            es[t] = ms; et[t] = mt;
        });
    for (auto& x : th) x.join();
    double ms = 0.0, mt = 0.0;
    for (unsigned t = 0; t < nt; t++) { if (!(es[t] <= ms)) ms = es[t]; if (!(et[t] <= mt)) mt = et[t]; }
    std::printf("sigmoid_max_abs_err %.9e\ntanh_max_abs_err %.9e\n", ms, mt);
    const float inf = INFINITY, nan = NAN;
    std::printf("sigmoid_pinf %.9e\nsigmoid_ninf %.9e\nsigmoid_nan %.9e\n", (double)hk_sigmoidf(inf), (double)hk_sigmoidf(-inf), (double)hk_sigmoidf(nan));
    std::printf("tanh_pinf %.9e\ntanh_ninf %.9e\ntanh_nan %.9e\n", (double)hk_tanhf_fast(inf), (double)hk_tanhf_fast(-inf), (double)hk_tanhf_fast(nan));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "--sweep")) return sweep();
    if (argc == 3) return run_case(argv[1], argv[2]);
    std::fprintf(stderr, "usage: %s CASE OUT | --sweep\n", argv[0]);
    return 2;
}
