// Host-side choosers of the k3 / k1 tap-list family (kernels: uad_convk16.inc, compiled in uad_conv_k3.hip): which launches the family takes, the tap lists of a
// data-path launch and the split of a filter gradient.  Included by the planner (uad_conv_plan.hip) and by tools/k3_ubench.hip.
#pragma once
#include <stdlib.h>
#include <string.h>
#include "uad_conv_launch.h"

// true when uad_launch_conv_f / _d run this kernel for the launch (bf16x3 planes given): k3, s1 (P 1) or s2 (P 0, big = 2 x small), identity
// activation on load, bias / addend epilogue, 32-channel contraction chunks, 64-channel output blocks, 8 x 8 position tiles
inline bool convk16_shape_ok(const UadConvDesc& d, bool f_type);
inline bool convk16_takes(const UadConvDesc& d, bool f_type, const UadXform& xf, const UadEpilogue& ep, const unsigned short* Wp16) {
    if (!Wp16 || xf.scale || ep.kind != UAD_EPI_BIAS || ep.mul) return false;
    return convk16_shape_ok(d, f_type);
}
inline bool convk16_shape_ok(const UadConvDesc& d, bool f_type) {
    static const bool off = getenv("UAD_NO_K3") != nullptr;
    if (off || (d.KS != 3 && d.KS != 1)) return false;
    const int CA = f_type ? d.CB : d.CS, Nn = f_type ? d.CS : d.CB;
    if (CA % 32 || Nn % 64 || d.HS % 8 || d.WS % 8) return false;
    const int P1 = d.KS == 3 ? 1 : 0;          // TF SAME: k3 s1 pads 1 before; k3 s2 on an even size and every k1 pad 0
    if (d.S == 1) return d.P == P1 && d.HB == d.HS && d.WB == d.WS;
    if (d.S == 2) return d.P == 0 && d.HB == 2 * d.HS && d.WB == 2 * d.WS;
    return false;
}

inline void run_convk16(const UadConvDesc& d, bool f_type, const float* in, float* out, const UadEpilogue& ep, const unsigned short* Wp16,
                        long long w16_plane, int planes, hipStream_t st) {
    ConvKArgs a;
    memset(&a, 0, sizeof a);
    a.A = in; a.Wp16 = Wp16; a.w16_plane = w16_plane; a.Out = out; a.bias = ep.bias; a.add = ep.add;
    a.N = d.N;
    if (d.KS == 1) {
        // one tap: small(i, j) = big(S i, S j) W (F), or big(S i, S j) = small(i, j) W^T (D; S 2: the other output pixels are bias + addend)
        a.toff[0] = 0; a.widx[0] = 0; a.y0 = a.x0 = 0; a.oy = a.ox = 0; a.MH = d.HS; a.MW = d.WS;
        if (f_type) {
            a.AH = d.HB; a.AW = d.WB; a.CA = d.CB; a.OH = d.HS; a.OW = d.WS; a.Nn = d.CS; a.os = 1;
            if (d.S == 1) uad_k3_launch(a, 1, 0, 1, planes, st); else uad_k3_launch(a, 2, 0, 1, planes, st);
        } else {
            a.AH = d.HS; a.AW = d.WS; a.CA = d.CS; a.OH = d.HB; a.OW = d.WB; a.Nn = d.CB; a.os = d.S;
            uad_k3_launch(a, 1, 0, 1, planes, st);
            if (d.S == 2) {
                const size_t total4 = (size_t)d.N * d.HB * d.WB * d.CB / 4;
                uad_k3_launch_k1s2_fill(out, ep.bias, ep.add, d.WB, d.CB, total4, st);
            }
        }
        return;
    }
    if (f_type) {
        // small(i, j) = sum big(S i - P + ky, S j - P + kx) W[ky, kx]
        a.AH = d.HB; a.AW = d.WB; a.CA = d.CB; a.MH = d.HS; a.MW = d.WS; a.OH = d.HS; a.OW = d.WS; a.Nn = d.CS;
        a.os = 1; a.oy = a.ox = 0; a.y0 = a.x0 = -d.P;
        const int IW = d.S * 7 + 3;
        for (int t = 0; t < 9; ++t) { a.toff[t] = (t / 3) * IW + (t % 3); a.widx[t] = t; }
        if (d.S == 1) uad_k3_launch(a, 1, 2, 9, planes, st); else uad_k3_launch(a, 2, 2, 9, planes, st);
        return;
    }
    a.AH = d.HS; a.AW = d.WS; a.CA = d.CS; a.OH = d.HB; a.OW = d.WB; a.Nn = d.CB;
    if (d.S == 1) {
        // big(Y, X) = sum small(Y + 1 - ky, X + 1 - kx) W[ky, kx]: halo origin -1, tap (ky, kx) at halo offset (2 - ky, 2 - kx)
        a.MH = d.HB; a.MW = d.WB; a.os = 1; a.oy = a.ox = 0; a.y0 = a.x0 = -1;
        const int IW = 7 + 3;
        for (int t = 0; t < 9; ++t) { a.toff[t] = (2 - t / 3) * IW + (2 - t % 3); a.widx[t] = t; }
        uad_k3_launch(a, 1, 2, 9, planes, st);
        return;
    }
    // S = 2: big(2 i + ky, 2 j + kx) <-> small(i, j).  Output-parity class (py, px), iteration (I, J) over the small grid writes big(2 I + py, 2 J + px):
    // even: ky 0 from small row I (halo row 1) and ky 2 from row I - 1 (halo row 0); odd: ky 1 from row I.  Halo origin -1, one extra row / column.
    a.MH = d.HS; a.MW = d.WS; a.os = 2; a.y0 = a.x0 = -1;
    const int IW = 7 + 2;
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) {
            int nt = 0;
            for (int ky = 0; ky < 3; ++ky) {
                if ((ky & 1) != py) continue;
                for (int kx = 0; kx < 3; ++kx) {
                    if ((kx & 1) != px) continue;
                    const int hy = ky == 2 ? 0 : 1, hx = kx == 2 ? 0 : 1;
                    a.toff[nt] = hy * IW + hx; a.widx[nt] = ky * 3 + kx; ++nt;
                }
            }
            a.oy = py; a.ox = px;
            if (nt == 4) uad_k3_launch(a, 1, 1, 4, planes, st);
            else if (nt == 2) uad_k3_launch(a, 1, 1, 2, planes, st);
            else uad_k3_launch(a, 1, 1, 1, planes, st);
        }
}

inline WK3Choice choose_wk3(const UadConvDesc& d) {
    WK3Choice c{false, 0, 0, 0, 0};
    static const bool off = getenv("UAD_NO_K3") != nullptr;
    if (off || d.KS != 3) return c;
    if (!((d.S == 1 && d.P == 1 && d.HB == d.HS && d.WB == d.WS) || (d.S == 2 && d.P == 0 && d.HB == 2 * d.HS && d.WB == 2 * d.WS))) return c;
    if (d.CB % 32 || d.CS % 64 || d.HS % 8 || d.WS % 8) return c;
    c.ncb = (d.S == 1 && d.CB % 64 == 0) ? 2 : 1;
    c.total_tiles = d.N * (d.HS / 8) * (d.WS / 8);
    const int blocks = (d.CB / (32 * c.ncb)) * (d.CS / 64);
    int splits = (512 + blocks - 1) / blocks;
    if (splits > c.total_tiles) splits = c.total_tiles;
    if (splits < 1) splits = 1;
    c.tiles_per_split = (c.total_tiles + splits - 1) / splits;
    c.splits = (c.total_tiles + c.tiles_per_split - 1) / c.tiles_per_split;
    c.ok = true;
    return c;
}
