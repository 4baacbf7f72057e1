// The row routine of the device graph generators (synth.hip: equal classes, one k and one d; synth_classes.hip: classes of any sizes
// with a k and a d each): both kernels give a wave a row and call sy_row, so where their definitions meet they write the same bits.
#pragma once
#include "philox.h"
#include "wdg_common.h"

namespace wdg {

constexpr int SY_MAX_N = 16384;          // GraphBatch's cap for a SELL-16 copy
constexpr int SY_THREADS = 256;          // up to four rows (waves) per workgroup
constexpr int SY_LDS_BYTES = 64 * 1024;  // of keys per workgroup: n <= 4096 -> 4 rows, n <= 8192 -> 2, else 1

__device__ __forceinline__ unsigned sy_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned sy_wave_inclusive(unsigned v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

// A wave per row.  Lane l owns the `cpl` = 4 x `per` consecutive candidate columns from l x cpl on (whole Philox blocks: a block
// serves four columns) and keeps their keys in LDS, column q of its range at word q x 64 + l of the wave's region: lane-private
// and conflict-free.  The k-th smallest key of the row's class block and the (d - k)-th smallest of the rest are found TOGETHER by
// a search over the 32 key bits, most significant first: T becomes the largest value with fewer than k keys below it, i.e. the
// k-th smallest key; a pass counts both groups in one walk over the lane's keys and sums the two counts packed in one word (each
// < 2^15 resp. <= 2^14).  Keys equal to the threshold are taken in column order until the group is full.  Lanes own ascending
// column ranges, so a prefix sum of the lanes' counts gives every chosen column its sorted position: no sort.
// (the row routine below: `cs`, `ce` = the row's class block, `k` / `n_other` = how many columns it takes inside / outside it, `D` =
// the row's length; it writes the row's columns and ones to col_out / val_out.  Wave-uniform arguments, no workgroup barrier.)
__device__ __forceinline__ void sy_row(unsigned *sy_lds, int wave, int lane, int per, int n, int row, int cs, int ce, int k, int n_other,
                                       int loops, int D, unsigned k0, unsigned k1, global_ptr<int32_t> col_out, global_ptr<float> val_out) {
    const int cpl = 4 * per, base = lane * cpl;
    unsigned *keys = sy_lds + static_cast<size_t>(wave) * cpl * 64 + lane;  // keys[q * 64]: column base + q
    const int cnt = max(0, min(n - base, cpl));                              // columns this lane owns
    for (int t = 0; 4 * t < cnt; ++t) {
        const philox_words w = philox4x32_10_words(static_cast<unsigned>(row), static_cast<unsigned>((base >> 2) + t), k0, k1);
#pragma unroll
        for (int x = 0; x < 4; ++x) keys[(4 * t + x) * 64] = w.w[x];  // (inside the lane's cpl slots, also past column n - 1)
    }
    // the lane's columns: [0, qa) and [qb, cnt) lie outside the row's class block, [qa, qb) inside; qi = the row itself
    const int qa = min(max(cs - base, 0), cnt), qb = min(max(ce - base, 0), cnt), qi = row - base;
    const bool self_here = qi >= 0 && qi < cnt;
    const unsigned key_i = self_here ? keys[qi * 64] : 0u;
    unsigned Ts = 0, To = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand_s = Ts | (1u << bit), cand_o = To | (1u << bit);
        unsigned a = 0, b = 0;
        for (int q = 0; q < qa; ++q) b += keys[q * 64] < cand_o ? 1u : 0u;
        for (int q = qa; q < qb; ++q) a += keys[q * 64] < cand_s ? 1u : 0u;
        for (int q = qb; q < cnt; ++q) b += keys[q * 64] < cand_o ? 1u : 0u;
        if (self_here && key_i < cand_s) --a;  // the row is no candidate of its own class
        const unsigned both = sy_wave_sum(b | (a << 16));
        if (static_cast<int>(both >> 16) < k) Ts = cand_s;
        if (static_cast<int>(both & 0xffffu) < n_other) To = cand_o;
    }
    // keys below the thresholds are in; of the keys equal to them, the first need_s / need_o in column order
    unsigned less_s = 0, less_o = 0, eq_s = 0, eq_o = 0;
    for (int q = 0; q < cnt; ++q) {
        const unsigned key = keys[q * 64];
        if (q >= qa && q < qb) {
            if (q != qi) less_s += key < Ts ? 1u : 0u, eq_s += key == Ts ? 1u : 0u;
        } else {
            less_o += key < To ? 1u : 0u, eq_o += key == To ? 1u : 0u;
        }
    }
    const unsigned less = sy_wave_sum(less_o | (less_s << 16));
    const int need_s = k - static_cast<int>(less >> 16), need_o = n_other - static_cast<int>(less & 0xffffu);
    const unsigned eq_mine = eq_o | (eq_s << 16), eq_before = sy_wave_inclusive(eq_mine, lane) - eq_mine;
    const int rank_s0 = static_cast<int>(eq_before >> 16), rank_o0 = static_cast<int>(eq_before & 0xffffu);
    auto walk = [&](bool write, int pos) {
        int rank_s = rank_s0, rank_o = rank_o0;
        for (int q = 0; q < cnt; ++q) {
            const unsigned key = keys[q * 64];
            bool in;
            if (q == qi) in = loops != 0;
            else if (q >= qa && q < qb) in = key < Ts || (key == Ts && rank_s++ < need_s);
            else in = key < To || (key == To && rank_o++ < need_o);
            if (in) {
                if (write && pos < D) col_out[pos] = base + q, val_out[pos] = 1.0f;
                ++pos;
            }
        }
        return pos;
    };
    const unsigned mine = static_cast<unsigned>(walk(false, 0));
    const unsigned before = sy_wave_inclusive(mine, lane) - mine;
    walk(true, static_cast<int>(before));
}

}  // namespace wdg
