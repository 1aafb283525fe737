// Host emulation of uad_resize2d and uad_mask_by_label (tests/test_resize_kernels_host.py): the kernel source of csrc/uad_resize.hip is
// compiled for the CPU (with -ffp-contract=off, as the device build) behind the shim of hip_host_emu.h.  Workgroups run one after the other; the
// threads of a workgroup are real threads around a std::barrier, because both kernels synchronise once after filling their LDS tables;
// the tables (`__shared__` = a static here) are poisoned before every workgroup.
// Driven by the library's own launch geometry (resize_grid / resize_block / resize_vec4, mask_label_grid / mask_label_vec4).
//   resize_emu resize in.f32 n_in h w idx.i32|- n H W mode out.f32
//   resize_emu mask vol.f32 labels.u8 n lut.u8 lesion_label want_lesion in_place out.f32 lesion.f32
#include "hip_host_emu.h"
#include "../../unsupervised_anomaly_detection_brain_mri_amd/csrc/uad_resize.hip"

// every table is filled with 0x7f bytes before each workgroup (as an index that is 2139062143, as a float a NaN), so that a kernel reading
// an entry its own workgroup never wrote goes visibly wrong
static void poison_lds() {
    memset(&rs_lds, 0x7f, sizeof(rs_lds));
    memset(ml_lut, 0x7f, sizeof(ml_lut));
}

static int run_resize(char** a) {
    const int n_in = atoi(a[1]), h = atoi(a[2]), w = atoi(a[3]), n = atoi(a[5]), H = atoi(a[6]), W = atoi(a[7]), mode = atoi(a[8]);
    if (n_in <= 0 || h <= 0 || w <= 0 || n <= 0 || H <= 0 || W <= 0) return 1;
    std::vector<float> in((size_t)n_in * h * w);
    if (!read_all(a[0], in)) return 2;
    std::vector<int> idx;
    if (strcmp(a[4], "-") != 0) {
        idx.resize(n);
        if (!read_all(a[4], idx)) return 2;
        for (int i : idx)
            if (i < 0 || i >= n_in) return 1;
    } else if (n != n_in) {
        return 1;
    }
    // the output sits between two guard rows that must come back untouched
    const size_t count = (size_t)n * H * W;
    Guarded<float, -777.0f> guarded(count);
    float* out = guarded.p;
    const int* ip = idx.empty() ? nullptr : idx.data();
    const float* inp = in.data();
    // the launch of uad_resize2d
    launch_threads(resize_grid(n, H, W), resize_block(), [&] { resize_kernel(inp, h, w, ip, H, W, mode, resize_vec4(W, out), out); }, poison_lds);
    if (!guarded.intact()) return 4;
    return write_all(a[9], out, count) ? 0 : 3;
}

static int run_mask(char** a) {
    const long long n = atoll(a[2]);
    const int lesion_label = atoi(a[4]), want_lesion = atoi(a[5]), in_place = atoi(a[6]);
    if (n <= 0) return 1;
    std::vector<float> vol(n), outv(n), lesion(n);
    std::vector<unsigned char> labels(n), lut(256);
    if (!read_all(a[0], vol) || !read_all(a[1], labels) || !read_all(a[3], lut)) return 2;
    float* out = in_place ? vol.data() : outv.data();
    float* les = want_lesion ? lesion.data() : nullptr;
    const float* v = vol.data();
    const unsigned char *lb = labels.data(), *lt = lut.data();
    // the launch of uad_mask_by_label
    launch_threads(mask_label_grid(n), dim3(ML_THREADS), [&] { mask_label_kernel(v, lb, n, lt, out, les, lesion_label, mask_label_vec4(v, lb, out, les)); }, poison_lds);
    if (!write_all(a[7], out, n)) return 3;
    if (want_lesion && !write_all(a[8], les, n)) return 3;
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 12 && strcmp(argv[1], "resize") == 0) return run_resize(argv + 2);
    if (argc == 11 && strcmp(argv[1], "mask") == 0) return run_mask(argv + 2);
    return 1;
}
