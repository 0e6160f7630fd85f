"""Record what the FP8 GEMM entry points would launch over a sweep of shapes -> tests/data/fp8_gemm_plans_parent.json.

Runs WITHOUT a GPU against a library built from a tree with docs/history/fp8_plan_trace.patch applied (and
-DSGLM_OPTIN_FUSIONS=1 on gemm_fp8.hip, so that the a16 entry point is there): the patched launchers format the launch they
would make into the line sgl_mi355_fp8_last_kernel() returns and launch nothing; pointers are fake and never read.

    SGL_MI355_LIB=<traced build>/libsgl_mi355.so python tools/fp8_plan_record.py tests/data/fp8_gemm_plans_parent.json
    python tools/fp8_plan_record.py --cases /tmp/cases.txt      # the sweep alone, one case per line (for a C++ driver)

No SGL_MI355_* knob may be set.  tests/test_fp8_plan_cpu.py holds ops.fp8_gemm_plan to every record."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS = [1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 1024, 2048, 4096, 8192]
LLAMA8B = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]
LLAMA70B_RANK = [(1280, 8192), (8192, 1024), (7168, 8192), (8192, 3584)]  # tests/test_gemm_exact_gpu.py
NS = [16, 128, 768, 6144, 7168, 12288, 12800, 20480, 28672]
KSTEPS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13, 16, 17, 27, 28, 30, 32, 64, 112]   # (9 = 3 x 3: the one-shot kernel's S = 3)
AMPLE = 1 << 40
KINDS = ("mm", "partials", "partials_a16", "silu_mul")
FIELDS = ("mb", "ph", "s", "nb", "wk", "exact", "nstage", "ri", "wm", "wn", "cb", "ks", "silu", "rawk", "scaled",
          "grid_x", "grid_y", "block", "lds", "sk", "per_slice", "waves", "groups", "raster_gn", "k_steps_per_slice", "finalize")
SLAB_FAMILIES = ("wstream_slab", "astat", "tiled3_rawk")


def shapes():
    """(N, K, a_pad, b_pad): pads are bytes added to the row strides."""
    out = [(n, k, 0, 0) for n, k in LLAMA8B + LLAMA70B_RANK + [(128256, 4096)]]
    out += [(n, 4096, 0, 0) for n in NS if (n, 4096) not in LLAMA8B]
    out += [(n, 14336, 0, 0) for n in (768, 7168)]                      # long K on narrow N: slabs at every row count
    out += [(4096, 128 * s, 0, 0) for s in KSTEPS if 128 * s not in (4096, 14336)]
    out += [(12800, 128 * s, 0, 0) for s in (4, 5, 8, 28)]              # the direct streamer's phase lengths
    out += [(1024, 65600, 0, 0), (20480, 576, 0, 0), (4096, 4096 + 16, 0, 0)]   # astat, astat_direct, a K tail
    out += [(28672, 4096, 0, 149808 - 4096)]                            # N * b_sn >= 2^32: per-lane weight offsets do not fit
    out += [(256, 512, (1 << 26) - 512, 0)]                             # M * a_sm >= 2^32 from 64 rows
    out += [(6144, 4096, 256, 0), (4096, 14336, 0, 128), (28672, 4096, 256, 128)]   # padded strides
    return out


def cases():
    """(kind, M, N, K, shuffled, a_pad, b_pad): every call the sweep makes, before the workspace variants."""
    for n, k, a_pad, b_pad in shapes():
        for shuffled in (0, 1):
            if shuffled and (k % 512 or n % 16 or b_pad):
                continue
            for m in MS:
                for kind in KINDS:
                    if kind == "silu_mul" and not (shuffled and n % 32 == 0):   # (its argument checks refuse the rest)
                        continue
                    yield kind, m, n, k, shuffled, a_pad, b_pad


class Recorder:
    def __init__(self):
        from sglang_npu_amd import _lib
        assert not [v for v in os.environ if v.startswith("SGL_MI355_") and v != "SGL_MI355_LIB"], "unset the SGL_MI355_* knobs"
        self._lib, self.lib = _lib, _lib.lib()
        self.lib.sgl_mi355_fp8_last_kernel.restype = ctypes.c_char_p

    def call(self, kind, M, N, K, shuffled, a_pad, b_pad, ws):
        """(rc, plan line or error text) of the real entry point; ws: -1 none, else floats."""
        z, vp, i = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
        fake = vp(0x10000)  # aligned, never dereferenced
        wsp, wsf = (fake, z(ws)) if ws >= 0 else (None, z(0))
        a_sm, b_sn = K + a_pad, K + b_pad
        sk = ctypes.c_int32(0)
        L = self.lib
        if kind == "mm" and shuffled:
            rc = L.sgl_mi355_fp8_scaled_mm_wshuffled(fake, fake, fake, fake, None, fake, wsp, wsf, z(M), z(N), z(K), z(a_sm), i(0), None)
        elif kind == "mm":
            rc = L.sgl_mi355_fp8_scaled_mm(fake, fake, fake, fake, None, fake, wsp, wsf, z(M), z(N), z(K), z(a_sm), z(b_sn), i(0), None)
        elif kind == "partials" and shuffled:
            rc = L.sgl_mi355_fp8_scaled_mm_partials_wshuffled(fake, fake, wsp, wsf, z(M), z(N), z(K), z(a_sm), ctypes.byref(sk), None)
        elif kind == "partials":
            rc = L.sgl_mi355_fp8_scaled_mm_partials(fake, fake, wsp, wsf, z(M), z(N), z(K), z(a_sm), z(b_sn), ctypes.byref(sk), None)
        elif kind == "partials_a16":  # the activation stride counts 16-bit elements and does not reach the plan
            rc = L.sgl_mi355_fp8_scaled_mm_partials_a16(fake, z(K), fake, fake, fake, i(shuffled), z(b_sn), wsp, wsf, z(M), z(N), z(K),
                                                        i(0), ctypes.byref(sk), None)
        else:
            rc = L.sgl_mi355_fp8_scaled_mm_silu_mul_wshuffled(fake, fake, fake, fake, None, fake, z(M), z(N), z(K), z(a_sm), i(0), None)
        if rc == 0:
            line = L.sgl_mi355_fp8_last_kernel().decode()
            assert line.startswith("family="), f"not a traced library: fp8_last_kernel() = {line!r}"
            kv = dict(t.split("=") for t in line.split())
            if kind.startswith("partials"):
                assert int(kv["sk"]) == sk.value, (line, sk.value)
            return 0, canonical(kv["family"], {k: int(v) for k, v in kv.items() if k != "family"})
        return rc, self._lib.last_error().replace(f"M={M} N={N} K={K}", "M={M} N={N} K={K}")


def canonical(family, ints):
    """One line per plan: the family and every non-zero field, in the struct's order."""
    assert set(ints) <= set(FIELDS), ints
    return " ".join([family] + [f"{f}={ints[f]}" for f in FIELDS if ints.get(f)])


def main():
    if sys.argv[1] == "--cases":
        with open(sys.argv[2], "w") as f:
            for kind, m, n, k, shuffled, a_pad, b_pad in cases():
                for ws in (-1, AMPLE):
                    f.write(f"{KINDS.index(kind)} {m} {n} {k} {k + a_pad} {k + b_pad} {shuffled} {int(ws >= 0)} {max(ws, 0)}\n")
        return
    rec = Recorder()
    plans, groups, nrows = {}, {}, 0
    for kind, m, n, k, shuffled, a_pad, b_pad in cases():
        tried = []
        if kind == "mm" and m <= 256:
            tried.append(-1)            # (above 256 rows run_gemm never looks at the workspace; the other kinds require one)
        tried.append(AMPLE if kind != "silu_mul" else -1)
        for ws in tried:
            rc, text = rec.call(kind, m, n, k, shuffled, a_pad, b_pad, ws)
            if rc == 1:                 # the entry point's own argument checks refuse the shape: not a dispatch decision
                continue
            assert rc in (0, 2), (rc, text)
            groups.setdefault((KINDS.index(kind), n, k, shuffled, a_pad, b_pad), []).append(
                [m, 0 if ws == AMPLE else ws, plans.setdefault((rc, text), len(plans))])
            nrows += 1
            if rc == 0 and ws == AMPLE and text.split()[0] in SLAB_FAMILIES:
                sk = int(dict(t.split("=") for t in text.split()[1:])["sk"])
                tried.append(sk * m * n - 1)   # exactly one float short of SK * M * N
    families = sorted({p.split()[0] for rc, p in plans if rc == 0})
    tiled2 = sorted({p.split(" grid_x")[0] for rc, p in plans if p.startswith("tiled2")})
    print(f"{nrows} records, {len(plans)} distinct plans; families reached: {families}; tiled2 forms: {tiled2}", file=sys.stderr)
    with open(sys.argv[1], "w") as f:
        f.write('{"group columns": ["kind", "N", "K", "shuffled", "a_pad", "b_pad", "calls"],\n')
        f.write(' "call columns": ["M", "workspace_floats (-1 none, 0 ample = 2^40)", "plan"],\n')
        f.write(' "kinds": %s,\n "plans (rc, plan or error text)": [\n' % json.dumps(KINDS))
        f.write(",\n".join("  " + json.dumps(p) for p in plans))
        f.write('\n ],\n "groups": [\n')
        f.write(",\n".join("  " + json.dumps(list(g) + [calls], separators=(",", ":")) for g, calls in groups.items()))
        f.write("\n ]}\n")


if __name__ == "__main__":
    main()
