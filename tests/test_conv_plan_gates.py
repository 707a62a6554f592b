"""The conv plan (csrc/model_shape.h) decides the five Winograd-or-fallback gates exactly as the five expressions it replaced
(copied here verbatim from the former model_infer.hip / model_train.hip), on both sides of every gate, with and without the
inference template utterance, and under SIR_CONV_FALLBACK unset / 1 / 2.  Host code only: compiled with the host compiler."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "speech-intent-recognizer_amd", "csrc")
SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "model_shape.h"
bool sir_conv_stage_fits(int conv, bool shape_ok) {          // api.hip
    static const int forced = getenv("SIR_CONV_FALLBACK") ? atoi(getenv("SIR_CONV_FALLBACK")) : 0;
    return shape_ok && forced < (conv == 2 ? 1 : 2);
}
int main() {
    const int bs[] = {1, 5, 256, 1100, 2621, 2622, 5242, 5243, 10485, 10486, 20971, 20972, 65535}, ts[] = {8, 200, 208, 2048};
    int bad = 0, side[5][2] = {};
    for (int tu = 0; tu < 2; ++tu) for (int t : ts) for (int B : bs) {
        SirDims d;
        if (!sir_make_dims(B, t, &d)) { printf("shape %d x %d rejected\n", B, t); return 2; }
        const SirConvPlan p = sir_conv_plan(&d, tu != 0);
        const int BF = B + tu;
        Wino2Geo geo2, geo3, g;
        const bool old[5] = {
            sir_conv_stage_fits(2, wino2_geo(BF, 32, d.wp1, 64, &geo2)) && sir_conv_stage_fits(3, wino2_geo(BF, 16, d.wp2, 128, &geo3)),
            sir_conv_stage_fits(2, wino2_geo(d.B, 32, d.wp1, 64, &g)), sir_conv_stage_fits(3, wino2_geo(d.B, 16, d.wp2, 128, &g)),
            sir_conv_stage_fits(2, (size_t)B * 32 * d.wp1 * 64 * 4 < ((size_t)1 << 31)), sir_conv_stage_fits(3, (size_t)B * 16 * d.wp2 * 128 * 4 < ((size_t)1 << 31))};
        const bool now[5] = {p.fwd_wino, p.dgrad2_wino, p.dgrad3_wino, p.wgrad2_wino, p.wgrad3_wino};
        for (int i = 0; i < 5; ++i) { bad += old[i] != now[i]; ++side[i][old[i]]; }
        printf("tu=%d t=%d B=%d: %d%d%d%d%d\n", tu, t, B, now[0], now[1], now[2], now[3], now[4]);
    }
    for (int i = 0; i < 5; ++i) printf("gate %d: closed %d open %d\n", i, side[i][0], side[i][1]);
    printf("mismatches %d\n", bad);
    return bad != 0;
}
"""


SRC_ONE = r"""
#include <cstdio>
#include <cstdlib>
#include "model_shape.h"
bool sir_conv_stage_fits(int conv, bool shape_ok) {          // api.hip
    static const int forced = getenv("SIR_CONV_FALLBACK") ? atoi(getenv("SIR_CONV_FALLBACK")) : 0;
    return shape_ok && forced < (conv == 2 ? 1 : 2);
}
int main(int argc, char** argv) {
    for (int i = 1; i + 1 < argc; i += 2) {
        SirDims d;
        if (!sir_make_dims(atoi(argv[i]), atoi(argv[i + 1]), &d)) return 2;
        const SirConvPlan p = sir_conv_plan(&d, false);
        printf("%d %d: %d%d%d%d%d\n", d.B, d.T, p.fwd_wino, p.dgrad2_wino, p.dgrad3_wino, p.wgrad2_wino, p.wgrad3_wino);
    }
    return 0;
}
"""


def test_first_gate_to_close_by_itself(tmp_path):
    """The training plan (fwd, dgrad2, dgrad3, wgrad2, wgrad3) with no switch: batch * t_frames = 524288 closes conv2's weight-gradient
    gate and nothing else -- (2048, 256), the shape test_conv_fallback_gpu.py runs for the nine-tap kernel -- one image less leaves
    every gate open, and conv3's weight gradient follows at twice the product."""
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    (tmp_path / "one.cpp").write_text(SRC_ONE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(tmp_path / "one.cpp"), "-o", str(tmp_path / "one")], check=True)
    env = {k: v for k, v in os.environ.items() if k != "SIR_CONV_FALLBACK"}
    shapes = [(2047, 256), (2048, 256), (256, 2048), (512, 1024), (4095, 256), (4096, 256)]
    r = subprocess.run([str(tmp_path / "one")] + [str(v) for s in shapes for v in s], env=env, capture_output=True, text=True, check=True)
    print(r.stdout)
    got = dict(line.split(": ") for line in r.stdout.splitlines())
    assert got == {"2047 256": "11111", "2048 256": "11101", "256 2048": "11101", "512 1024": "11101", "4095 256": "11101",
                   "4096 256": "11100"}


@pytest.mark.parametrize("fallback", [None, "1", "2"])
def test_plan_gates_equal_the_expressions_they_replaced(fallback, tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    (tmp_path / "gates.cpp").write_text(SRC)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(tmp_path / "gates.cpp"), "-o", str(tmp_path / "gates")], check=True)
    env = {k: v for k, v in os.environ.items() if k != "SIR_CONV_FALLBACK"}
    if fallback:
        env["SIR_CONV_FALLBACK"] = fallback
    r = subprocess.run([str(tmp_path / "gates")], env=env, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    sides = [line.split() for line in r.stdout.splitlines() if line.startswith("gate ")]
    assert len(sides) == 5
    for i, s in enumerate(sides):               # both sides of every gate the switch leaves open
        forced_shut = fallback == "2" or (fallback == "1" and i in (0, 1, 3))
        assert int(s[3]) > 0 and (forced_shut or int(s[5]) > 0), s
