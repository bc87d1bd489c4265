// Test infrastructure: the forward ray's (cell, heading sector) lists (hk_env_params.h build_ray_lists) and their walk (hk_env_device.h
// ray_list_min) on the host, through the stand-in <hip/hip_runtime.h> in tests/host_emu, against a scan of every wall with the same ray_seg.
// Poses: a few hundred per grid cell that lists walls, plus random ones anywhere on the grid; headings as phase_assemble forms them (sincos of
// a yaw, atan2 of the forward); speeds from 0 to the handle's top speed; straight and curve.
//
// in : <file>  int32 header[6] = {magic, sizeof(hk_config), L, NW, poses per cell, seed}, hk_config, sections, walls
// out: stdout  "key value" pairs: rl_sectors, entries, bytes, poses, mismatches (predicates), value_mismatches (bit equality)
#include <hip/hip_runtime.h>
#include <random>
#include <string>
#include <vector>

thread_local hk_emu_dim3 threadIdx;
hk_emu_dim3 blockIdx, blockDim, gridDim;
namespace hk_emu { Barrier bar; uint64_t slot[LANES]; unsigned char* dyn_shared; }

#include "hk_env_params.h"

using namespace hk;

template <class T> static std::vector<T> read_n(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: ray_lists_host_check <in>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const auto hd = read_n<int32_t>(f, 6);
    if (hd[0] != 0x484b4532 || hd[1] != (int)sizeof(hk_config)) { std::fprintf(stderr, "bad header\n"); return 2; }
    const int L = hd[2], NW = hd[3], per_cell = hd[4];
    hk_config cfg = read_n<hk_config>(f, 1)[0];
    auto sec_in = read_n<hk_section>(f, L);
    auto wall_in = read_n<hk_wall_seg>(f, NW);
    std::fclose(f);
    cfg.sections = sec_in.data(); cfg.walls = wall_in.data();
    EnvParams P;
    std::vector<hk_section> sections; std::vector<hk_wall_seg> walls; std::vector<unsigned char> pk; std::vector<int> perms; std::string err;
    if (int rc = env_build_params(cfg, sections, walls, P, pk, perms, err)) { std::fprintf(stderr, "env_build_params: %d %s\n", rc, err.c_str()); return 2; }
    P.tab = pk.data();
    const TabView T = tab_view(P, pk.data());
    std::printf("rl_sectors %d\n", P.rl_sectors);
    if (!P.rl_sectors) return 0;
    const size_t ncell = (size_t)P.grid_nx * P.grid_nz;
    std::printf("entries %u\nbytes %d\n", T.rl_off[ncell * P.rl_sectors], (int)pk.size() - P.tab_bytes);

    std::mt19937 rng((uint32_t)hd[5]);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    long long poses = 0, bad = 0, bad_value = 0;
    auto check = [&](float px, float pz) {
        const float yaw = U(rng) * 6.2831853f, speed = U(rng) * P.st.TopSpeed;
        float fx, fz;
        hk_sincosf(yaw, &fx, &fz);
        float heading = hk_atan2f(fz, fx);                    // phase_assemble's heading and origin (HKA:734, MLAgent_Sensors)
        if (heading < 0) heading += TWO_PI_F;
        const float ox = px + SENSOR_LZ * fx, oz = pz + SENSOR_LZ * fz;
        float dx, dz;
        sensor_dir(P, 0, fx, fz, dx, dz);
        float scan = 3.0e38f;
        for (const hk_wall_seg& w : walls) {
            const float t = ray_seg_host(ox, oz, dx, dz, w);
            if (t >= 0.0f && t < scan) scan = t;
        }
        for (int straight = 0; straight < 2; straight++) {
            const float thr = straight ? 8.0f : 5.0f;
            const float lo = f_min(speed * 0.5f, thr), hi = f_max(speed * 0.5f, thr);
            const float walk = ray_list_min(P, T, ox, oz, dx, dz, heading, lo, hi);
            poses++;
            if ((walk <= speed * 0.5f) != (scan <= speed * 0.5f) || (walk <= thr) != (scan <= thr)) {
                if (bad < 5) std::fprintf(stderr, "predicates: p (%.9g, %.9g) yaw %.9g speed %.9g straight %d: walk %.9g scan %.9g\n", px, pz, yaw, speed, straight, walk, scan);
                bad++;
            }
            // without the stop on decided comparisons the walk returns the scan's value wherever a comparison can see it
            const float full = ray_list_min(P, T, ox, oz, dx, dz, heading, -1.0f, hi);
            if (scan <= hi && full != scan) {
                if (bad_value < 5) std::fprintf(stderr, "value: p (%.9g, %.9g) yaw %.9g hi %.9g: walk %.9g scan %.9g\n", px, pz, yaw, hi, full, scan);
                bad_value++;
            }
        }
    };
    const unsigned short* goff = T.grid_off;
    for (int iz = 0; iz < P.grid_nz; iz++)
        for (int ix = 0; ix < P.grid_nx; ix++) {
            const size_t c = (size_t)iz * P.grid_nx + ix;
            if (goff[c + 1] == goff[c]) continue;          // cells that list walls
            for (int n = 0; n < per_cell; n++)
                check(P.grid_x0 + (ix + U(rng)) * GRID_CELL, P.grid_z0 + (iz + U(rng)) * GRID_CELL);
        }
    for (int n = 0; n < per_cell * 200; n++)
        check(P.grid_x0 + U(rng) * P.grid_nx * GRID_CELL, P.grid_z0 + U(rng) * P.grid_nz * GRID_CELL);
    std::printf("poses %lld\nmismatches %lld\nvalue_mismatches %lld\n", poses, bad, bad_value);
    return 0;
}
