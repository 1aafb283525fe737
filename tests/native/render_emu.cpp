// Host emulation of uad_render_minmax_u8, uad_render_heatmap and uad_render_overlay (tests/test_render_kernels_host.py): the kernel source
// of csrc/uad_render.hip is compiled for the CPU (with -ffp-contract=off, as the device build) behind the shim of hip_host_emu.h.  Workgroups run one
// after the other; the threads of a workgroup are real threads around a std::barrier (the reduction of the two normalising kernels
// synchronises twice per slice) and live for the whole launch; the LDS structs (`__shared__` = a static here) are poisoned before every
// workgroup.  Driven by the library's own launch geometry (render_path / render_block / render_grid / *_vec_*, overlay_grid / overlay_vec).
// in_off shifts the base of every input by that many ELEMENTS off its 16-byte alignment, out_off the base of the output by that many
// BYTES, so that the alignment fallbacks run; the output sits between guard bytes that must come back untouched.
//   render_emu grey x.f32 n hw in_off out_off out.u8
//   render_emu heat d.f32 n h w lut.u8 in_off out_off out.u8
//   render_emu overlay x.f32 pred.f32 gt.u8 n hw in_off out_off out.u8
#include "hip_host_emu.h"
#include "../../unsupervised_anomaly_detection_brain_mri_amd/csrc/uad_render.hip"

// 0x7f bytes: as a float or a double a NaN, as a colour a wrong one
static void poison_lds() {
    memset(&rn_grey_lds, 0x7f, sizeof(rn_grey_lds));
    memset(&rn_heat_lds, 0x7f, sizeof(rn_heat_lds));
}

using GuardedOut = Guarded<unsigned char, 0xa5>;

static int run_grey(char** a) {
    const int n = atoi(a[1]), hw = atoi(a[2]), in_off = atoi(a[3]), out_off = atoi(a[4]);
    if (n <= 0 || hw <= 0 || in_off < 0 || out_off < 0) return 1;
    const size_t count = (size_t)n * hw;
    Shifted<float> x(count, in_off);
    if (!read_all(a[0], x.p, count)) return 2;
    GuardedOut out(count, out_off);
    const float* xp = x.p;
    unsigned char* op = out.p;
    // the launch of uad_render_minmax_u8
    const int path = render_path(hw), vi = render_vec_in(xp, hw), vo = grey_vec_out(op, hw);
    if (path == RN_PATH_SMALL) launch_threads(render_grid(n), render_block(path), [&] { minmax_u8_kernel<RN_SMALL, true>(xp, n, hw, vi, vo, op); }, poison_lds);
    else if (path == RN_PATH_LARGE) launch_threads(render_grid(n), render_block(path), [&] { minmax_u8_kernel<RN_LARGE, true>(xp, n, hw, vi, vo, op); }, poison_lds);
    else launch_threads(render_grid(n), render_block(path), [&] { minmax_u8_kernel<RN_LARGE, false>(xp, n, hw, vi, vo, op); }, poison_lds);
    if (!out.intact()) return 4;
    return write_all(a[5], op, count) ? 0 : 3;
}

static int run_heat(char** a) {
    const int n = atoi(a[1]), h = atoi(a[2]), w = atoi(a[3]), in_off = atoi(a[5]), out_off = atoi(a[6]);
    if (n <= 0 || h <= 0 || w <= 0 || in_off < 0 || out_off < 0 || out_off % 4) return 1;
    const long long hw = (long long)h * w;
    const size_t count = (size_t)n * hw;
    Shifted<float> d(count, in_off);
    Shifted<unsigned char> lut(1024, in_off);
    if (!read_all(a[0], d.p, count) || !read_all(a[4], lut.p, (size_t)1024)) return 2;
    GuardedOut out(count * 4, out_off);
    const float* dp = d.p;
    const unsigned char* lp = lut.p;
    unsigned char* op = out.p;
    // the launch of uad_render_heatmap
    const int path = heat_path(hw), vi = render_vec_in(dp, hw), vo = heat_vec_out(op, hw);
    if (path == RN_PATH_SMALL) launch_threads(render_grid(n), render_block(path), [&] { heatmap_kernel<RN_SMALL, true>(dp, n, h, w, lp, vi, vo, op); }, poison_lds);
    else launch_threads(render_grid(n), render_block(path), [&] { heatmap_kernel<RN_LARGE, false>(dp, n, h, w, lp, vi, vo, op); }, poison_lds);
    if (!out.intact()) return 4;
    return write_all(a[7], op, count * 4) ? 0 : 3;
}

static int run_overlay(char** a) {
    const int n = atoi(a[3]), hw = atoi(a[4]), in_off = atoi(a[5]), out_off = atoi(a[6]);
    if (n <= 0 || hw <= 0 || in_off < 0 || out_off < 0) return 1;
    const size_t count = (size_t)n * hw;
    Shifted<float> x(count, in_off), pred(count, in_off);
    Shifted<unsigned char> gt(count, in_off);
    if (!read_all(a[0], x.p, count) || !read_all(a[1], pred.p, count) || !read_all(a[2], gt.p, count)) return 2;
    GuardedOut out(count * 3, out_off);
    const float *xp = x.p, *pp = pred.p;
    const unsigned char* gp = gt.p;
    unsigned char* op = out.p;
    const long long total = (long long)count;
    // the launch of uad_render_overlay
    const int vec = overlay_vec(xp, pp, gp, op);
    launch_threads(overlay_grid(total), dim3(OV_THREADS), [&] { overlay_kernel(xp, pp, gp, total, vec, op); }, poison_lds);
    if (!out.intact()) return 4;
    return write_all(a[7], op, count * 3) ? 0 : 3;
}

int main(int argc, char** argv) {
    if (argc == 8 && strcmp(argv[1], "grey") == 0) return run_grey(argv + 2);
    if (argc == 10 && strcmp(argv[1], "heat") == 0) return run_heat(argv + 2);
    if (argc == 10 && strcmp(argv[1], "overlay") == 0) return run_overlay(argv + 2);
    return 1;
}
