// Host emulation of uad_histogram_by_class (tests/test_histograms_kernels_host.py): the kernel source of csrc/uad_hist.hip is compiled for
// the CPU (with -ffp-contract=off, as the device build) behind the shim of hip_host_emu.h.  Workgroups run one after the other; the threads of a
// workgroup are real threads around a std::barrier (the tree reduction synchronises nine times per tile) and live for the whole launch; the
// LDS struct (`__shared__` = a static here) is poisoned before every workgroup, the workspace of partials before the launch.  Driven by the
// library's own launch geometry (hc_tiles / hc_grid / hc_lab_vec); max_blocks > 0 caps the grid below the library's, which must not change a
// bit of the sums.  in_off shifts the base of the values by that many ELEMENTS off its 16-byte alignment, lab_off the base of the class
// ids by that many BYTES, so that the guarded head / tail chunks and the byte loads of the ids run.
//   hist_emu in.f32 lab.u8 n n_classes edges.f32|- bins centre.f64|- moments in_off lab_off max_blocks out.bin
// out.bin: counts int64 [n_classes * bins], class_count int64 [n_classes], sums fp64 [n_classes] (the last two only with moments = 1).
#include "hip_host_emu.h"
#include "../../unsupervised_anomaly_detection_brain_mri_amd/csrc/uad_hist.hip"

static void poison_lds() { memset(&hc_lds, 0xff, sizeof(hc_lds)); }

int main(int argc, char** argv) {
    if (argc != 13) return 1;
    const long long n = atoll(argv[3]);
    const int n_classes = atoi(argv[4]), bins = atoi(argv[6]), moments = atoi(argv[8]), in_off = atoi(argv[9]), lab_off = atoi(argv[10]),
              max_blocks = atoi(argv[11]);
    if (n <= 0 || n_classes < 1 || n_classes > HC_CLASSES || bins < 0 || bins > UAD_HISTOGRAM_MAX_BINS || in_off < 0 || in_off > 3 || lab_off < 0) return 1;
    Shifted<float> in(n, in_off);
    Shifted<uint8_t> lab(n, lab_off);
    if (!read_all(argv[1], in.p, (size_t)n) || !read_all(argv[2], lab.p, (size_t)n)) return 2;
    std::vector<float> edges(bins + 1);
    if (bins > 0 && !read_all(argv[5], edges.data(), (size_t)bins + 1)) return 2;
    std::vector<double> centre(n_classes);
    const bool centred = strcmp(argv[7], "-") != 0;
    if (centred && !read_all(argv[7], centre.data(), (size_t)n_classes)) return 2;

    // the launches of uad_histogram_by_class
    const unsigned long long tiles = hc_tiles((unsigned long long)n);
    unsigned grid = hc_grid(tiles);
    if (max_blocks > 0 && (unsigned)max_blocks < grid) grid = (unsigned)max_blocks;
    std::vector<unsigned long long> counts((size_t)n_classes * bins + 1, 0ull);
    std::vector<HcPartial> partials(tiles);
    memset(partials.data(), 0xff, tiles * sizeof(HcPartial));           // every tile's partial must be written
    std::vector<long long> class_count(n_classes, -1);
    std::vector<double> sums(n_classes, NAN);
    const float* ip = in.p;
    const uint8_t* lp = lab.p;
    const float* ep = bins > 0 ? edges.data() : nullptr;
    const double* cp = centred ? centre.data() : nullptr;
    HcPartial* pp = moments ? partials.data() : nullptr;
    const int lab_vec = hc_lab_vec(ip, lp);
    launch_threads(dim3(grid), dim3(HC_THREADS),
                   [&] { hist_class_kernel(ip, lp, (unsigned long long)n, n_classes, ep, bins, cp, counts.data(), pp, tiles, lab_vec); }, poison_lds);
    if (moments)
        launch_threads(dim3(1), dim3(HC_THREADS), [&] { hist_class_finish_kernel(pp, tiles, n_classes, class_count.data(), sums.data()); }, poison_lds);

    FILE* f = fopen(argv[12], "wb");
    if (!f) return 3;
    bool ok = fwrite(counts.data(), sizeof(long long), (size_t)n_classes * bins, f) == (size_t)n_classes * bins;
    if (moments) {
        ok = ok && fwrite(class_count.data(), sizeof(long long), n_classes, f) == (size_t)n_classes;
        ok = ok && fwrite(sums.data(), sizeof(double), n_classes, f) == (size_t)n_classes;
    }
    fclose(f);
    return ok ? 0 : 3;
}
