// Host emulation of uad_shifted_sums and uad_clamp_standardize (tests/test_standardize_kernels_host.py): the kernel source of
// csrc/uad_moments.hip is compiled for the CPU (with -ffp-contract=off, as the device build) behind the shim of hip_host_emu.h.  Workgroups run
// one after the other; the threads of a workgroup are real threads around a std::barrier (the tree reduction synchronises nine times per tile);
// the LDS struct is poisoned before every workgroup, the workspace of partials before the launch (every tile's partial must be written); the
// two sums and the map's output lie between guards.  Driven by the library's own launch geometry (ms_tiles / ms_grid / ms_map_vec /
// ms_map_grid); max_blocks > 0 caps the grid below the library's, which must not change a bit.  in_off shifts the base of the values by
// that many ELEMENTS off its 16-byte alignment, out_off the base of the map's output.  The float arguments come as their BIT PATTERNS
// (unsigned decimal), so that no text conversion stands between the test's numbers and the kernel's.
//   moments_emu in.f32 n in_off out_off lo hi shift centre mean sd max_blocks out.bin
// out.bin: sums fp64 [2], then the map fp32 [n].  The map is run a second time in place (out == in) and must give the same bytes (exit 4).
#include "hip_host_emu.h"
#include "../../unsupervised_anomaly_detection_brain_mri_amd/csrc/uad_moments.hip"

static void poison_lds() { memset(&ms_lds, 0xff, sizeof(ms_lds)); }

static float bits(const char* s) {
    const uint32_t u = (uint32_t)strtoul(s, nullptr, 10);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv) {
    if (argc != 13) return 1;
    const long long n = atoll(argv[2]);
    const int in_off = atoi(argv[3]), out_off = atoi(argv[4]), max_blocks = atoi(argv[11]);
    const float lo = bits(argv[5]), hi = bits(argv[6]), shift = bits(argv[7]), centre = bits(argv[8]), mean = bits(argv[9]), sd = bits(argv[10]);
    if (n <= 0 || n > MS_MAX_N || in_off < 0 || in_off > 3 || out_off < 0 || out_off > 3) return 1;
    Shifted<float> in(n, in_off);
    if (!read_all(argv[1], in.p, (size_t)n)) return 2;

    // the launches of uad_shifted_sums
    const unsigned long long tiles = ms_tiles((unsigned long long)n);
    unsigned grid = ms_grid(tiles);
    if (max_blocks > 0 && (unsigned)max_blocks < grid) grid = (unsigned)max_blocks;
    std::vector<MsPartial> partials(tiles);
    memset(partials.data(), 0xff, tiles * sizeof(MsPartial));
    Guarded<double, -777.0> sums(2);
    const float* ip = in.p;
    launch_threads(dim3(grid), dim3(MS_THREADS), [&] { shifted_sums_kernel(ip, (unsigned long long)n, lo, hi, shift, centre, partials.data(), tiles); },
                   poison_lds);
    launch_threads(dim3(1), dim3(MS_THREADS), [&] { shifted_sums_finish_kernel(partials.data(), tiles, sums.p); }, poison_lds);
    if (!sums.intact()) return 5;

    // the launch of uad_clamp_standardize, out of place and in place
    Guarded<float, -777.0f> out(n, out_off);
    int vec = ms_map_vec(ip, out.p);
    unsigned mgrid = ms_map_grid((unsigned long long)n, vec);
    if (max_blocks > 0 && (unsigned)max_blocks < mgrid) mgrid = (unsigned)max_blocks;
    launch_loop(dim3(mgrid), dim3(256), [&] { clamp_standardize_kernel(ip, (unsigned long long)n, lo, hi, mean, sd, out.p, vec); });
    if (!out.intact()) return 5;
    Guarded<float, -777.0f> inplace(n, in_off);
    memcpy(inplace.p, ip, (size_t)n * sizeof(float));
    vec = ms_map_vec(inplace.p, inplace.p);
    mgrid = ms_map_grid((unsigned long long)n, vec);
    launch_loop(dim3(mgrid), dim3(256), [&] { clamp_standardize_kernel(inplace.p, (unsigned long long)n, lo, hi, mean, sd, inplace.p, vec); });
    if (!inplace.intact()) return 5;
    if (memcmp(inplace.p, out.p, (size_t)n * sizeof(float)) != 0) return 4;

    FILE* f = fopen(argv[12], "wb");
    if (!f) return 3;
    bool ok = fwrite(sums.p, sizeof(double), 2, f) == 2;
    ok = ok && fwrite(out.p, sizeof(float), (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok ? 0 : 3;
}
