// Host emulation of uad_brain_boxes / uad_brain_boxes_f32 and uad_assemble_batch (tests/test_batch_kernels_host.py): the kernel source of
// csrc/uad_batch.hip -- with the generator of csrc/uad_kernels.h, which is all that header gives a host emulation -- is compiled for the CPU
// (with -ffp-contract=off, as the device build) behind the shim of hip_host_emu.h.  The boxes kernel reduces through LDS: its workgroups run one
// after the other, the threads of a workgroup are real threads around a std::barrier, and the LDS (`__shared__` = a static here) is poisoned
// before every workgroup.  The assemble kernel has no barrier and runs as a plain loop.  Every output sits between guard words that must come
// back untouched.  Driven by the library's own launch geometry (boxes_grid / boxes_block, assemble_grid / assemble_block / assemble_args).
//   batch_emu boxes_u8 labels.u8 byte_offset n H W lut.u8|- out.i32        (byte_offset: the label store's base, off its 16-byte alignment)
//   batch_emu boxes_f32 masks.f32 n H W out.i32
//   batch_emu assemble src.f32 N idx.i32|- n H W C rects.i32|- sigma seed step sample0 rng_stream want_x out_x.f32 out_ce.f32
#include "hip_host_emu.h"
#include "../../unsupervised_anomaly_detection_brain_mri_amd/csrc/uad_batch.hip"

// 0x7f bytes: as a box entry 2139062143, as a LUT entry "set" -- a kernel reading LDS its own workgroup never wrote goes visibly wrong
static void poison_lds() { memset(&bb_lds, 0x7f, sizeof(bb_lds)); }

static int run_boxes_u8(char** a) {
    const int off = atoi(a[1]), n = atoi(a[2]), H = atoi(a[3]), W = atoi(a[4]);
    if (n <= 0 || H <= 0 || W <= 0 || off < 0 || off > 15) return 1;
    const size_t count = (size_t)n * H * W;
    Shifted<unsigned char> labels(count, off);
    if (!read_all(a[0], labels.p, count)) return 2;
    std::vector<unsigned char> lut;
    if (strcmp(a[5], "-") != 0) {
        lut.resize(256);
        if (!read_all(a[5], lut)) return 2;
    }
    Guarded<int, -777> guarded((size_t)n * 4);
    int* out = guarded.p;
    const unsigned char *lb = labels.p, *lt = lut.empty() ? nullptr : lut.data();
    // the launch of uad_brain_boxes
    launch_threads(boxes_grid(n), boxes_block(), [&] { brain_boxes_kernel<unsigned char>(lb, H, W, lt, out); }, poison_lds);
    if (!guarded.intact()) return 4;
    return write_all(a[6], out, (size_t)n * 4) ? 0 : 3;
}

static int run_boxes_f32(char** a) {
    const int n = atoi(a[1]), H = atoi(a[2]), W = atoi(a[3]);
    if (n <= 0 || H <= 0 || W <= 0) return 1;
    std::vector<float> masks((size_t)n * H * W);
    if (!read_all(a[0], masks)) return 2;
    Guarded<int, -777> guarded((size_t)n * 4);
    int* out = guarded.p;
    const float* m = masks.data();
    // the launch of uad_brain_boxes_f32
    launch_threads(boxes_grid(n), boxes_block(), [&] { brain_boxes_kernel<float>(m, H, W, nullptr, out); }, poison_lds);
    if (!guarded.intact()) return 4;
    return write_all(a[4], out, (size_t)n * 4) ? 0 : 3;
}

static int run_assemble(char** a) {
    const int N = atoi(a[1]), n = atoi(a[3]), H = atoi(a[4]), W = atoi(a[5]), C = atoi(a[6]);
    const float sigma = strtof(a[8], nullptr);
    const unsigned long long seed = strtoull(a[9], nullptr, 10), step = strtoull(a[10], nullptr, 10);
    const long long sample0 = atoll(a[11]);
    const int rng_stream = atoi(a[12]), want_x = atoi(a[13]);
    if (N <= 0 || n <= 0 || H <= 0 || W <= 0 || C <= 0 || ((long long)H * W * C) % 4 || !(sigma >= 0.0f) || sample0 < 0) return 1;
    const size_t per = (size_t)H * W * C;
    Shifted<float> src(N * per, 0);
    if (!read_all(a[0], src.p, N * per)) return 2;
    std::vector<int> idx, rects;
    if (strcmp(a[2], "-") != 0) {
        idx.resize(n);
        if (!read_all(a[2], idx)) return 2;
        for (int i : idx)
            if (i < 0 || i >= N) return 1;
    } else if (n != N) {
        return 1;
    }
    if (strcmp(a[7], "-") != 0) {
        rects.resize((size_t)n * 12);
        if (!read_all(a[7], rects)) return 2;
    }
    if (!want_x && rects.empty()) return 1;
    Guarded<float, -777.0f> gx(n * per), gce(n * per);
    float* out_x = want_x ? gx.p : nullptr;
    float* out_ce = rects.empty() ? nullptr : gce.p;
    // the launch of uad_assemble_batch
    const AssembleArgs args = assemble_args(src.p, idx.empty() ? nullptr : idx.data(), H, W, C, rects.empty() ? nullptr : rects.data(), sigma, seed, step,
                                            sample0, rng_stream, out_x, out_ce);
    launch_loop(assemble_grid(n, args.quads), assemble_block(), [&] { assemble_kernel(args); });
    if (!gx.intact() || !gce.intact()) return 4;
    if (!want_x)                                                    // an output that was not asked for stays untouched
        for (size_t i = 0; i < n * per; ++i)
            if (gx.p[i] != -777.0f) return 4;
    if (rects.empty())
        for (size_t i = 0; i < n * per; ++i)
            if (gce.p[i] != -777.0f) return 4;
    if (want_x && !write_all(a[14], out_x, n * per)) return 3;
    if (out_ce && !write_all(a[15], out_ce, n * per)) return 3;
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 9 && strcmp(argv[1], "boxes_u8") == 0) return run_boxes_u8(argv + 2);
    if (argc == 7 && strcmp(argv[1], "boxes_f32") == 0) return run_boxes_f32(argv + 2);
    if (argc == 18 && strcmp(argv[1], "assemble") == 0) return run_assemble(argv + 2);
    return 1;
}
