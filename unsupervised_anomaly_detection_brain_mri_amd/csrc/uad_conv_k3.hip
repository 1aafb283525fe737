// The k3 / k1 tap-list family (uad_convk16.inc): data-path kernels, filter gradient, the k1 s2 fill and the HIP-event profile table of their launches.
// uad_conv_plan.hip decides what runs (uad_conv_k3_plan.h) and calls the uad_k3_launch* functions below.
#include <string.h>
#include <map>
#include <array>
#include <string>
#include <vector>
#include "uad_gemm_common.h"

namespace {
#include "uad_convk16.inc"
}  // namespace

#define UAD_K3_CASE(s, e, n) if (sin == s && ext == e && ntaps == n) { launch_convk16<s, e, n>(a, planes, st); return; }
void uad_k3_launch(const ConvKArgs& a, int sin, int ext, int ntaps, int planes, hipStream_t st) {
    UAD_K3_CASE(1, 0, 1) UAD_K3_CASE(2, 0, 1)                          // k1 s1 / s2
    UAD_K3_CASE(1, 2, 9) UAD_K3_CASE(2, 2, 9)                          // k3 s1 / s2, whole tap list
    UAD_K3_CASE(1, 1, 4) UAD_K3_CASE(1, 1, 2) UAD_K3_CASE(1, 1, 1)     // k3 s2 D kind: one output-parity class
    fprintf(stderr, "uad: no tap-list instance <%d, %d, %d>\n", sin, ext, ntaps); abort();
}
#undef UAD_K3_CASE

void uad_k3_launch_k1s2_fill(float* out, const float* bias, const float* add, int OW, int Nn, size_t total4, hipStream_t st) {
    hipLaunchKernelGGL(k1s2_fill_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, out, bias, add, OW, Nn, total4);
}

void uad_k3_launch_w(const ConvWArgs& a, const WK3Choice& c, int S, int ncb, hipStream_t st) {
    if (S == 1) { if (ncb == 2) launch_convk_w16<1, 2>(a, c, st); else launch_convk_w16<1, 1>(a, c, st); }
    else launch_convk_w16<2, 1>(a, c, st);
}

void uad_k3_prof_enable(bool on) {
    if (on && !g_k3prof) { for (auto& r : g_k3recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); } g_k3recs.clear(); }
    g_k3prof = on;
}
// one text line per launch shape: "kind p1 p2 ntaps npl N MH MW CA Nn calls total_ms form"; returns the number of bytes the full table needs
int uad_k3_prof_read(char* buf, int cap) {
    (void)hipDeviceSynchronize();
    std::map<std::array<int, 11>, std::pair<int, double>> agg;
    for (auto& r : g_k3recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
        std::array<int, 11> k;
        for (int i = 0; i < 11; ++i) k[i] = r.key[i];
        auto& e = agg[k];
        e.first += 1; e.second += ms;
    }
    std::string out;
    char line[256];
    for (auto& kv : agg) {
        int n = 0;
        for (int i = 0; i < 10; ++i) n += snprintf(line + n, sizeof line - n, "%d ", kv.first[i]);
        snprintf(line + n, sizeof line - n, "%d %.6f %d\n", kv.second.first, kv.second.second, kv.first[10]);
        out += line;
    }
    if (buf && cap > 0) { const size_t c = out.size() < (size_t)cap - 1 ? out.size() : (size_t)cap - 1; memcpy(buf, out.data(), c); buf[c] = 0; }
    return (int)out.size() + 1;
}
