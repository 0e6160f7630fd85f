"""CPU: the FP8 GEMM dispatch rule (csrc/gemm_fp8_plan.h fp8_plan, seen through ops.fp8_gemm_plan) launches what the
ladder of launchers it replaced launched.

tests/data/fp8_gemm_plans_parent.json is the record: the commit before the rule became one function, with
docs/history/fp8_plan_trace.patch applied, driven through the real entry points over the sweep of
tools/fp8_plan_record.py with no knob set -- family, template selectors, grid, block, LDS bytes and the kernels' runtime
integers of every launch, or the return code and error text of every refusal.  Nothing here needs a GPU."""
import json
import os

from conftest import ROOT
from sglang_npu_amd import ops
import exact_gemm as eg

with open(os.path.join(ROOT, "tests", "data", "fp8_gemm_plans_parent.json")) as _f:
    _REC = json.load(_f)
KINDS, PLANS = _REC["kinds"], _REC["plans (rc, plan or error text)"]
# one row per recorded call: [kind, M, N, K, shuffled, a_pad, b_pad, workspace, plan] (the file groups the calls of a shape)
ROWS = [[kind, M, N, K, shuffled, a_pad, b_pad, ws, plan]
        for kind, N, K, shuffled, a_pad, b_pad, calls in _REC["groups"] for M, ws, plan in calls]
AMPLE = 1 << 40


def _plan(row):
    kind, M, N, K, shuffled, a_pad, b_pad, ws, _ = row
    return ops.fp8_gemm_plan(M, N, K, bool(shuffled), AMPLE if ws == 0 else max(ws, 0), KINDS[kind], K + a_pad, K + b_pad)


def _line(p) -> str:
    """The record's form of a plan: the family and every non-zero field in the struct's order."""
    return " ".join([p.family] + [f"{n}={v}" for n, v in zip(p._fields[3:], p[3:]) if v])


_ALL = [(row, _plan(row)) for row in ROWS]  # computed once, shared by the tests below


def test_every_recorded_launch_and_refusal_is_reproduced_field_for_field():
    bad = []
    for row, p in _ALL:
        rc, text = PLANS[row[-1]]
        got = _line(p) if p.rc == 0 else p.error
        want = text if rc == 0 else text.format(M=row[1], N=row[2], K=row[3])
        if (p.rc, got) != (rc, want):
            bad.append(f"{KINDS[row[0]]} {row[1:8]}: recorded ({rc}) {want!r}, plan ({p.rc}) {got!r}")
    assert not bad, f"{len(bad)} of {len(ROWS)} records differ:\n" + "\n".join(bad[:20])


def test_the_sweep_reaches_every_family_and_every_late_decline():
    fams = {p.family for _, p in _ALL if p.rc == 0}
    assert fams == {"skinny", "oneshot", "astat", "astat_direct", "wstream", "wstream_slab", "tiled", "tiled2", "tiled3", "tiled3_ks2",
                    "tiled3_silu", "tiled3_rawk"}
    # tiled2: 84, 22 and 2 are the forms the rule picks by itself; 48, 8 and the fall-back form need SGL_MI355_TILED_V2
    assert {(p.nstage, p.ri, p.wm, p.wn) for _, p in _ALL if p.family == "tiled2"} == {(2, 8, 2, 4), (3, 2, 4, 2), (2, 4, 2, 2)}
    by_case = {tuple(row[:8]): p for row, p in _ALL}
    mm = KINDS.index("mm")
    # 32-bit weight offsets (N * b_sn >= 2^32): the streamer, astat_direct and the one-shot kernel all decline -> astat
    # (64-bit offsets) where there is a workspace, skinny where there is none
    assert by_case[(mm, 16, 28672, 4096, 0, 0, 149808 - 4096, 0)].family == "astat"
    assert by_case[(mm, 16, 28672, 4096, 0, 0, 149808 - 4096, -1)].family == "skinny"
    assert by_case[(mm, 16, 28672, 4096, 0, 0, 0, 0)].family == "wstream"
    # a workspace one float short of SK * M * N: the slab form declines and the next rung takes the shape
    short = [(row, p) for row, p in _ALL if row[7] > 0]
    assert len(short) > 100 and not any(p.family in ("wstream_slab", "astat", "tiled3_rawk") for _, p in short)
    assert {p.family for row, p in short if row[0] == mm} >= {"oneshot", "skinny", "tiled2", "wstream"}
    # no phase length divides K / 128 (PH == 0), and the a16 fill's single-phase rule
    assert by_case[(mm, 64, 12800, 640, 0, 0, 0, 0)].family == "oneshot"
    a16 = KINDS.index("partials_a16")
    # (64 rows x 28672 columns: 224 groups leave one K slice of four 8-step phases)
    assert by_case[(a16, 16, 4096, 4096, 1, 0, 0, 0)].per_slice == 1 and by_case[(a16, 64, 28672, 4096, 1, 0, 0, 0)].rc == 2


def test_the_tests_own_statements_of_the_rule_agree_with_the_plan():
    """exact_gemm.fp8_tiled_variant / fp8_oneshot_split are what tests/test_gemm_exact_gpu.py names its cases by."""
    v2 = {(3, 2, 4, 2): 22, (2, 8, 2, 4): 84, (3, 4, 4, 2): 48, (3, 8, 2, 2): 8, (2, 4, 2, 2): 2}
    checked = {"tiled": 0, "oneshot": 0}
    for row, p in _ALL:
        kind, M, N, K, shuffled = row[:5]
        if KINDS[kind] != "mm" or p.rc:
            continue
        if p.family in ("tiled", "tiled2", "tiled3", "tiled3_ks2"):
            variant = {"tiled": "tiled", "tiled2": f"tiled2 {v2.get((p.nstage, p.ri, p.wm, p.wn))}", "tiled3_ks2": f"tiled3_ks2 cb={p.cb}",
                       "tiled3": "tiled3 256x256" if p.wm == 2 else f"tiled3 128x{64 * p.cb}"}[p.family]
            assert eg.fp8_tiled_variant(M, N, K, bool(shuffled)) == variant, row
            checked["tiled"] += 1
        elif p.family == "oneshot":
            assert eg.fp8_oneshot_split(K // 128) == p.s and p.s * p.wk == K // 128, row
            checked["oneshot"] += 1
    assert min(checked.values()) > 100, checked
    assert {p.s for _, p in _ALL if p.family == "oneshot"} == {1, 2, 3, 4}


def test_default_workspace_is_what_fp8_scaled_mm_passes():
    """workspace_floats=None: the pool's floor or _fp8_slab_floats, whichever is larger, up to 256 rows; none above."""
    for M, N, K in [(64, 4096, 14336), (128, 28672, 4096), (256, 4096, 14336), (257, 4096, 14336)]:
        want = max(ops._fp8_workspace.floor, ops._fp8_slab_floats(M, N, K)) if M <= 256 else 0
        assert ops.fp8_gemm_plan(M, N, K, True) == ops.fp8_gemm_plan(M, N, K, True, workspace_floats=want)
    assert ops.fp8_gemm_plan(64, 4096, 14336, True).family == "wstream_slab"
    assert ops.fp8_gemm_plan(64, 4096, 14336, True, workspace_floats=0).family != "wstream_slab"
