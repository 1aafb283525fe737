// Host emulation of uad_confusion_by_segment (tests/test_confusion_kernels_host.py): the kernel source of csrc/uad_confusion.hip is compiled
// for the CPU behind the shim of hip_host_emu.h.  Workgroups run one after the other; the threads of a workgroup are real threads around a
// std::barrier (the tree reduction synchronises nine times) and live for the whole launch; the LDS struct (`__shared__` = a static here) is
// poisoned before every workgroup, and the counts hold garbage before the first launch, so the zeroing kernel is part of what is proven.
// Driven by the library's own launch geometry (cf_grid_zero / cf_grid_x / cf_grid_tn) once for every entry of the comma-separated list
// `blocks`: 0 = the library's workgroups per segment, b > 0 = b workgroups per segment instead (fewer than tiles: a workgroup strides over
// several; more than one: the atomics of several workgroups meet) -- the counts must not depend on it.  pred_off shifts the base of the values by that many ELEMENTS off its 16-byte
// alignment, gt_off the base of the labels by that many BYTES.
//   confusion_emu pred.f32 gt.u8 n offsets.i64 n_segments thr pred_off gt_off blocks out.bin
// out.bin: counts int64 [n_segments * 4] per entry of `blocks`, in its order.
#include "hip_host_emu.h"
#include "../../unsupervised_anomaly_detection_brain_mri_amd/csrc/uad_confusion.hip"

static void poison_lds() { memset(&cf_lds, 0xff, sizeof(cf_lds)); }

int main(int argc, char** argv) {
    if (argc != 11) return 1;
    const long long n = atoll(argv[3]);
    const int n_segments = atoi(argv[5]), pred_off = atoi(argv[7]), gt_off = atoi(argv[8]);
    const float thr = (float)atof(argv[6]);
    if (n <= 0 || n_segments < 1 || n_segments > CF_MAX_SEGMENTS || pred_off < 0 || pred_off > 3 || gt_off < 0) return 1;
    Shifted<float> pred(n, pred_off);
    Shifted<uint8_t> gt(n, gt_off);
    std::vector<long long> offsets((size_t)n_segments + 1);
    if (!read_all(argv[1], pred.p, (size_t)n) || !read_all(argv[2], gt.p, (size_t)n) || !read_all(argv[4], offsets)) return 2;
    long long max_len = 0;
    for (int s = 0; s < n_segments; ++s) {
        if (offsets[s] < 0 || offsets[s + 1] < offsets[s] || offsets[s + 1] > n) return 1;
        max_len = std::max(max_len, offsets[s + 1] - offsets[s]);
    }

    const float* pp = pred.p;
    const uint8_t* gp = gt.p;
    FILE* f = fopen(argv[10], "wb");
    if (!f) return 3;
    bool ok = true;
    for (const char* b = argv[9]; b && *b; b = strchr(b, ',') ? strchr(b, ',') + 1 : nullptr) {
        const int blocks = atoi(b);
        if (blocks < 0 || blocks > 64) return 1;
        // the launches of uad_confusion_by_segment
        std::vector<unsigned long long> counts((size_t)n_segments * 4, 0xdeadbeefdeadbeefull);
        const unsigned grid = blocks > 0 ? (unsigned)blocks : cf_grid_x(max_len, n_segments);
        launch_loop(dim3(cf_grid_zero(n_segments)), dim3(CF_THREADS), [&] { confusion_zero_kernel(n_segments, counts.data()); });
        launch_threads(dim3(grid, (unsigned)n_segments), dim3(CF_THREADS), [&] { confusion_kernel(pp, thr, gp, n, offsets.data(), counts.data()); }, poison_lds);
        launch_loop(dim3(cf_grid_tn(n_segments)), dim3(CF_THREADS), [&] { confusion_tn_kernel(n, offsets.data(), n_segments, counts.data()); });
        ok = ok && fwrite(counts.data(), sizeof(unsigned long long), counts.size(), f) == counts.size();
    }
    fclose(f);
    return ok ? 0 : 3;
}
