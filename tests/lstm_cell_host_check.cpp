// lstm_cell_host_check.cpp — hk_lstm_cell alone on the host: the SAME HK_HD definition the kernels compile (csrc/hk_policy_lstm.h), applied to
// given gate pre-activations.  The bf16 recurrent chain (hk.h "RECURRENT ACTORS IN BF16") keeps the cell fp32 and unchanged, so the composed
// reference of tests/test_lstm_bf16_gpu.py takes its gates from the device tap and its cell from here.  Built by tests/lstm_bf16_restate.py
// with policy_lstm_twin's flags.
//   usage: lstm_cell_host_check in.bin out.bin
//   in : int32 magic, rows, m; float z [rows][4m] (gates i f g o), float c [rows][m]        out: float h' [rows][m], float c' [rows][m]
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../hierarchicalkarting_amd/csrc/hk_policy_lstm.h"

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t hd[3];
    if (std::fread(hd, sizeof(int32_t), 3, f) != 3 || hd[0] != 0x4C43454C || hd[1] < 0 || hd[2] < 1) { std::fprintf(stderr, "bad header\n"); return 2; }
    const size_t rows = (size_t)hd[1], m = (size_t)hd[2];
    std::vector<float> z(rows * 4 * m), c(rows * m), out(2 * rows * m);
    if (std::fread(z.data(), sizeof(float), z.size(), f) != z.size() || std::fread(c.data(), sizeof(float), c.size(), f) != c.size()) {
        std::fprintf(stderr, "short input\n");
        return 2;
    }
    std::fclose(f);
    for (size_t r = 0; r < rows; r++)
        for (size_t u = 0; u < m; u++) {
            const float* zr = &z[r * 4 * m];
            hk_lstm_cell(zr[u], zr[m + u], zr[2 * m + u], zr[3 * m + u], c[r * m + u], &out[r * m + u], &out[rows * m + r * m + u]);
        }
    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    const bool ok = std::fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
