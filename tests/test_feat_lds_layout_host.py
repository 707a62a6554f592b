"""The LDS layouts of the three frame kernels (csrc/feat_lds.h) against the hand sums and the pointer carves they replaced (copied
here verbatim from the former features.hip): every total equals the launch site's old sum, the regions follow each other without
gap or overlap in the old order and the last one ends at the total, every offset keeps its alignment (8 bytes for the complex and
double regions, 16 for the tap table), and the totals at 1026 filter weights stay below the 160 KB of a workgroup.  Nothing checked
the host's sum against the kernel's carve before; here one struct is both.  Host code only: compiled with the host compiler."""
import os
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "speech-intent-recognizer_amd", "csrc")
SRC = r"""
#include <cstdio>
#include <cstdint>
#include "feat_lds.h"
struct float2 { float x, y; };
struct MelTap { int fa; float wa; int fb; float wb; };
static const int XS = 72;                                    // wave_fft.h (a device header); feat_common.h ties it to XBUF: static_assert(XBUF == 8 * XS)
static int bad = 0;
struct Region { const char* name; int word_off; size_t bytes; size_t align; };
static void walk(const char* kernel, int mel_nnz, const Region* r, int n, size_t total, size_t old_sum) {
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        const size_t off = (size_t)r[i].word_off * 4;
        if (off != at) { printf("%s mel_nnz=%d: %s at %zu, the carve has it at %zu\n", kernel, mel_nnz, r[i].name, off, at); ++bad; }
        if (off % r[i].align) { printf("%s mel_nnz=%d: %s at %zu is not %zu-byte aligned\n", kernel, mel_nnz, r[i].name, off, r[i].align); ++bad; }
        at = off + r[i].bytes;
    }
    if (at != total) { printf("%s mel_nnz=%d: the last region ends at %zu, total %zu\n", kernel, mel_nnz, at, total); ++bad; }
    if (total != old_sum) { printf("%s mel_nnz=%d: total %zu, the old sum %zu\n", kernel, mel_nnz, total, old_sum); ++bad; }
    printf("%s mel_nnz=%d: %zu bytes\n", kernel, mel_nnz, total);
}
int main() {
    const int nnzs[] = {0, 1, 3, 4, 5, 513, 1023, 1024, 1025, 1026, 3840}, r1s[] = {2, 4, 8};
    for (int mel_nnz : nnzs) {
        const size_t melw = (size_t)((mel_nnz + 3) & ~3) * sizeof(float);          // melw + ((tb.mel_nnz + 3) & ~3)
        {   // feat_utt_kernel: sir_features_launch's sum, the kernel's carve
            const size_t lds = (size_t)NW * XBUF * sizeof(float2) + NW * sizeof(double) + (size_t)2 * NW * PROW * sizeof(float) +
                               (size_t)((mel_nnz + 3) & ~3) * sizeof(float) + (1024 + 8 * TW2S) * sizeof(float2);
            const FeatUttLds l(mel_nnz);
            const Region r[] = {{"xall", l.xall, (size_t)NW * XBUF * sizeof(float2), 8}, {"red", l.red, NW * sizeof(double), 8},
                                {"Pbuf", l.pbuf, (size_t)2 * NW * PROW * sizeof(float), 4}, {"melw", l.melw, melw, 4},
                                {"winl", l.tail() + l.winl, 512 * sizeof(float2), 8}, {"twul", l.tail() + l.twul, 512 * sizeof(float2), 8},
                                {"tw2l", l.tail() + l.tw2l, 8 * TW2S * sizeof(float2), 8}};
            walk("feat_utt_kernel", mel_nnz, r, 7, l.bytes(), lds);
            if (mel_nnz == 1026 && l.bytes() >= 160 * 1024) { printf("feat_utt_kernel: %zu bytes at 1026\n", l.bytes()); ++bad; }
        }
        {   // feat_utt_bwd_kernel: sir_features_bwd_launch's sum, the kernel's carve
            const size_t lds = (size_t)NW * XBUF * sizeof(float2) + NW * sizeof(double) + (size_t)NW * PROW * sizeof(float) +
                               (size_t)NW * DMS * sizeof(float) + 512 * sizeof(float) + 516 * sizeof(MelTap) +
                               (size_t)((mel_nnz + 3) & ~3) * sizeof(float) + (1024 + 8 * TW2S + 512) * sizeof(float2);
            const FeatUttBwdLds l(mel_nnz);
            const Region r[] = {{"xall", l.xall, (size_t)NW * XBUF * sizeof(float2), 8}, {"red", l.red, NW * sizeof(double), 8},
                                {"P", l.p, (size_t)NW * PROW * sizeof(float), 4}, {"dmt", l.dmt, (size_t)NW * DMS * sizeof(float), 4},
                                {"carry", l.carry, 512 * sizeof(float), 4}, {"tapl", l.tapl, 516 * sizeof(MelTap), 16},
                                {"melw", l.melw, melw, 4}, {"winl", l.tail() + l.winl, 512 * sizeof(float2), 8},
                                {"twul", l.tail() + l.twul, 512 * sizeof(float2), 8}, {"tw2l", l.tail() + l.tw2l, 8 * TW2S * sizeof(float2), 8},
                                {"tw1l", l.tail() + l.tw1l, 512 * sizeof(float2), 8}};
            walk("feat_utt_bwd_kernel", mel_nnz, r, 11, l.bytes(), lds);
            if (mel_nnz == 1026 && l.bytes() >= 160 * 1024) { printf("feat_utt_bwd_kernel: %zu bytes at 1026\n", l.bytes()); ++bad; }
        }
        for (int R1 : r1s) {   // feat_gen_frames_kernel<R1>: sir_features_gen_lds_bytes(n_fft = 128 R1), the kernel's carve
            const int n_fft = 128 * R1;
            const int n = n_fft / 2, r1 = n / 64;
            const size_t lds = (size_t)NW * r1 * XS * sizeof(float2) + (size_t)2 * NW * (n + 2) * sizeof(float) +
                               (size_t)((mel_nnz + 3) & ~3) * sizeof(float) + (size_t)3 * n * sizeof(float2);
            const int N = 64 * R1, XB = R1 * XS, PR = N + 2;
            const FeatGenLds l(R1, mel_nnz);
            const Region r[] = {{"xall", l.xall, (size_t)NW * XB * sizeof(float2), 8}, {"Pbuf", l.pbuf, (size_t)2 * NW * PR * sizeof(float), 4},
                                {"melw", l.melw, melw, 4}, {"winl", l.tail() + l.winl, N * sizeof(float2), 8},
                                {"twnl", l.tail() + l.twnl, N * sizeof(float2), 8}, {"twul", l.tail() + l.twul, N * sizeof(float2), 8}};
            char name[64];
            snprintf(name, sizeof name, "feat_gen_frames_kernel<%d>", R1);
            walk(name, mel_nnz, r, 6, l.bytes(), lds);
            if (mel_nnz == 1026 && l.bytes() >= 160 * 1024) { printf("%s: %zu bytes at 1026\n", name, l.bytes()); ++bad; }
        }
    }
    printf("mismatches %d\n", bad);
    return bad != 0;
}
"""


def test_layouts_equal_the_sums_and_carves_they_replaced(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    (tmp_path / "lds.cpp").write_text(SRC)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(tmp_path / "lds.cpp"), "-o", str(tmp_path / "lds")], check=True)
    r = subprocess.run([str(tmp_path / "lds")], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "mismatches 0"
    assert len(lines) == 1 + 11 * (2 + 3)           # every (kernel, mel_nnz) pair was walked
