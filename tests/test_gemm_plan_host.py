"""CPU: the GEMM family's routing (csrc/gemm.hip ed_gemm_plan) run DRY through ``edgedict_gemm_plan`` - no device,
nothing launched, the pointers are made-up addresses of which only alignment and nullness count - against
tests/golden/gemm_plans.json: for every case the whole record (kernel id, grid, block, dynamic LDS bytes, K slices,
K per slice, zero pass, reduce pass, vendor try).  The expected records are the decisions of the build BEFORE the
planner existed, taken with a recording switch at each of its launch sites; the cases sit on both sides of every edge
of the chain.  Switches that are read once per process (and, for uniformity, the per-call one) run in a child process."""
import ctypes
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gemm_plans.json")
# The records assume 256 compute units: what the library falls back to without a device, and the MI355X's count.
WORDS = 9
DTYPE = {"f32": 0, "bf16": 1}


def plan(lib, c):
    """The record of one case (a dict of tests/golden/gemm_plans.json)."""
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    rec = (ctypes.c_int32 * WORDS)()
    rc = lib.edgedict_gemm_plan(DTYPE[c["dtype_in"]], DTYPE[c["dtype_out"]], vp(c["A"]), ll(c["lda"]), c["a_kmajor"],
                                vp(c["B"]), ll(c["ldb"]), c["b_kmajor"], vp(c["C"]), ll(c["ldc"]), c["M"], c["N"],
                                c["K"], vp(c["bias1"]), vp(c["bias2"]), c["accumulate"], c["split_k"],
                                c["max_wg_per_cu"], vp(c["partials"]), c["lse"], c["unreduced"], rec)
    assert rc == 0, c["name"]
    return list(rec)


def _cases():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_cases_reach_every_kernel_and_vendor_route():
    cs = _cases()
    assert {c["record"][0] for c in cs} == set(range(15))
    assert {c["record"][8] for c in cs} == {0, 1, 2, 3}
    assert any(c["record"][6] for c in cs) and any(c["record"][7] for c in cs)


def test_default_routing_matches_the_recorded_decisions(hip_lib):
    got = {c["name"]: plan(hip_lib, c) for c in _cases() if not c["env"]}
    want = {c["name"]: c["record"] for c in _cases() if not c["env"]}
    assert len(want) > 70
    assert got == want


def test_switched_routing_matches_the_recorded_decisions(hip_lib):
    from edgedict_amd import _lib
    groups = {}
    for c in _cases():
        if c["env"]:
            groups.setdefault(json.dumps(c["env"], sort_keys=True), []).append(c)
    assert len(groups) >= 8
    for key, grp in groups.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("EDGEDICT_")}
        env.update(json.loads(key))
        r = subprocess.run([sys.executable, __file__, _lib.LIB_PATH], input=json.dumps(grp), env=env,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert json.loads(r.stdout) == [c["record"] for c in grp], key


def test_rejected_arguments_come_back_as_a_status(hip_lib):
    c = dict(_cases()[0], split_k=0)
    rec = (ctypes.c_int32 * WORDS)()
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    rc = hip_lib.edgedict_gemm_plan(0, 0, vp(c["A"]), ll(c["lda"]), 1, vp(c["B"]), ll(c["ldb"]), 1, vp(c["C"]),
                                    ll(c["ldc"]), c["M"], c["N"], c["K"], None, None, 0, 0, 0, None, 0, 0, rec)
    assert rc == -1 and b"split_k" in hip_lib.edgedict_last_error()


if __name__ == "__main__":      # child of test_switched_routing...: cases on stdin, records on stdout
    child_lib = ctypes.CDLL(sys.argv[1])
    print(json.dumps([plan(child_lib, c) for c in json.loads(sys.stdin.read())]))
