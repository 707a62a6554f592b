"""The fallback generation of the conv2 / conv3 kernels at their own shape edges, and at the first shape that chooses one for real.

csrc/model_shape.h sends a conv stage that does not fit 32-bit offsets to bf16x6_kernels.h (direct 3x3), conv_wino_bf16x6_kernel.h
(first-generation Winograd), wgrad_bf16x6_kernel.h (nine-tap weight gradient) and, in ragged inference, the mask pass of
infer_tables.h.  The test-only SIR_CONV_FALLBACK (1 = conv2's stages, 2 = every stage) is read once per process: every group of
cases (tests/fallback_cases.py) runs in a fresh child under ``timeout``, one after another, and the next child is not started
once one has failed, timed out or died on a signal.  References and bounds are the suite's own, unchanged (fallback_cases.py's
docstring): bf16x6 is specified as fp32-accurate, so the fallbacks get no tolerance of their own.

Training shapes (batch 1 to 3; wp1 = t / 2, wp2 = t / 4 are the map widths the conv2 / conv3 stages see):
  t = 8, 9, 10, 12, 14, 15   wp1 mod 4 = 0, 0, 1, 2, 3, 3: every residue of the first-generation Winograd's 4-pixel block; odd t drops a pool column
  t = 23, 31                 wp1 = 11, 15; wp2 = 5, 7
  t = 36, 60, 64, 68         wp2 = 9, 15, 16, 17: around the direct kernel's 8-pixel tile and dgrad3's 8-pixel block
  t = 130                    wp1 = 65: one pixel past a 16-pixel k-step of the nine-tap kernel
  t = 256, 257               wp1 = 128 = wgrad_x6_max_w(64), wp2 = 64 = wgrad_x6_max_w(128): the widest rows the nine-tap kernel takes
  (17, 8), (33, 15)          many images, tiny map
  dfeats wanted at t = 9, 15, 68, 257 (the chain through the direct dgrad2); dropout 0.5 at (3, 36).

The refusal (SIR_CONV_FALLBACK=2): a row wider than that -- t >= 258 for conv2, >= 260 for conv3 -- with the stage's Winograd gate
closed is SIR_EUNSUPPORTED from every backward entry point before the first launch (it used to come from inside the chain, behind
the head and GRU kernels); a frozen conv weight needs no nine-tap launch and runs.  By itself the gate closes at batch * t_frames >=
524288 (conv2) / 1048576 (conv3): include/sir_hip.h at "Sequence regimes".

The natural gate: batch 2048 of 256 frames is the smallest batch x length at which the nine-tap kernel is both chosen
(2048 * 32 * 128 * 64 * 4 = 2^31: wgrad2_wino closed, every other gate open -- tests/test_conv_plan_gates.py) and able to run.

Measured on an MI355X (worst of the 29 gradients, max |a - b| / rms, SIR_CONV_FALLBACK = 2 / 1; bound 2e-3; in brackets dfeats):

    t     batch  worst gradient       |  t     batch  worst gradient
    8     1      1.3e-5 / 1.3e-5      |  36    3      1.1e-5 / 1.1e-5   (dropout 0.5: 1.1e-5 / 1.1e-5)
    8     17     1.0e-5 / 1.0e-5      |  60    2      7.1e-6 / 7.1e-6
    9     2      1.3e-5 / 1.3e-5  (3.3e-6 / 3.6e-6)   64    1      1.0e-5 / 1.0e-5
    10    3      1.2e-5 / 1.2e-5      |  68    3      7.4e-6 / 8.4e-6   (4.4e-6 / 4.6e-6)
    12    1      2.8e-5 / 2.8e-5      |  130   2      1.1e-5 / 6.0e-6
    14    2      1.5e-5 / 1.5e-5      |  256   1      1.4e-5 / 8.7e-6
    15    3      1.7e-5 / 1.7e-5  (3.9e-6 / 3.3e-6)   257   2      1.0e-5 / 8.8e-6   (4.1e-6 / 4.1e-6)
    15    33     1.0e-5 / 1.0e-5      |
    23    2      1.3e-5 / 1.3e-5      |
    31    1      1.3e-5 / 1.3e-5      |

Loss within 4.9e-7, logits 1.4e-7, norms 1.8e-6, stage gradients 6.4e-6 * rms everywhere: the figures of the default kernels
(test_token_range_gpu.py).  Frozen BatchNorm dfeats 3.3e-6 .. 3.6e-6 * rms.  Dense inference: at most 8.4e-8 at init scale and 3.1e-6
under the sharp head at 8 .. 31 frames, 2.2e-7 / 8.6e-6 at 2055 frames; pad-skipped batches 6.4e-8, ragged 6.4e-8; the same under
both values.  Operand range: fallback_cases.group_range's docstring and include/sir_hip.h.  The refused shapes: forward logits
within 1.2e-7; (1, 520) with frozen conv weights: dfeats 4.1e-6 * rms, worst of the 26 wanted gradients 5.6e-6 * rms.
Natural gate, (2048, 256): max |got - ref| / rms(ref) = 7.5e-5 for conv2.weight's gradient (rms 8.2e-4; loss scale 2^19, the
step itself 0.05 s), status word clean.
Wall time: every child 3 to 4 s, start-up of the process included (the bodies of the groups 0.6 to 1.6 s, the natural one 3.8 s);
the whole module, twelve children, 40 s.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import fallback_cases
fallback_cases.main({group!r})
"""
# (group of fallback_cases.py, time limit in seconds)
SWITCHED = [("train_short", 120), ("train_tiles", 150), ("variants", 120), ("infer", 150), ("range", 120)]


_FAILED = []                 # children that failed, timed out or died: nothing more is started on the GPU from this module


def _child(tmp_path, group, limit, fallback):
    """One group in a fresh process under its own time limit; asserts on the return code and the final token."""
    assert not _FAILED, f"not started: an earlier child of this module failed {_FAILED}"
    _FAILED.append((group, fallback))
    script = tmp_path / f"fallback_{group}.py"
    script.write_text(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=os.path.join(ROOT, "tests", "golden"), group=group))
    env = {k: v for k, v in os.environ.items() if k != "SIR_CONV_FALLBACK"}
    if fallback is not None:
        env["SIR_CONV_FALLBACK"] = fallback
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, str(script)], capture_output=True, text=True, env=env, cwd=ROOT)
    print(r.stdout[-20000:])
    assert r.returncode == 0 and f"FALLBACK-CASES-OK {group}" in r.stdout, (group, fallback, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    _FAILED.pop()


@pytest.mark.parametrize("group,limit", SWITCHED, ids=[g for g, _ in SWITCHED])
@pytest.mark.parametrize("fallback", ["2", "1"])
def test_fallback_kernels_at_their_shape_edges(tmp_path, fallback, group, limit):
    """Training step, backward variants, dense / pad-skipped / ragged inference and the two operand-range cases, every conv stage
    (2) or conv2's stages (1) on the fallback kernels: one child per group, in turn; none is started once one has failed."""
    _child(tmp_path, group, limit, fallback)


def test_backward_refuses_a_row_the_nine_tap_kernel_cannot_hold(tmp_path):
    """(1, 258), (1, 260), (2, 520) with every gate closed: the forward runs (logits against the oracle), every backward entry point
    returns SIR_EUNSUPPORTED with zero launches, sentinel-filled gradients and dfeats and the workspace bit for bit as they were,
    and a clean status word; (1, 520) with the conv weights frozen and dfeats wanted runs, against the oracle."""
    _child(tmp_path, "refusal", 150, "2")


def test_nine_tap_weight_gradient_where_the_plan_chooses_it(tmp_path):
    """Batch 2048 of 256 frames, no switch: conv2.weight's gradient against dz2 (x) a1 summed in float64 on the device, within
    range_ref.GRAD_BOUND * rms; loss and all 29 gradients finite; sir_check_status SIR_OK (no recurrence timed out)."""
    _child(tmp_path, "natural", 300, None)
