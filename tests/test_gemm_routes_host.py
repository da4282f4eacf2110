"""CPU: tests/test_gemm_gpu.py tests the kernels it names.  Every product of that file is an entry of tests/gemm_cases.py;
here each entry is planned DRY through ``ops.gemm_plan`` on meta tensors (no device, nothing launched - the same
argument marshalling as ``ops.gemm``) and held to the kernel id, K slices and vendor word it expects, and the table as a
whole to reaching every kernel of default routing - gemm_tn256.hip at its ragged edges, on its item walk and with a
short last K slice.  The records assume 256 compute units: the library's fallback without a device and the MI355X's
count; only the grid depends on it, and it is used in one inequality."""
import pytest

import gemm_cases
from gemm_cases import CASES


@pytest.fixture(scope="module")
def records(hip_lib):
    return {name: gemm_cases.plan_on_meta(c) for name, c in CASES.items()}


def test_every_entry_plans_to_its_expected_route(records):
    wrong = {}
    for name, c in CASES.items():
        rec = records[name]
        if rec[0] != c.kernel or (c.split is not None and rec[4] != c.split) or \
                (c.vendor is not None and rec[8] != c.vendor):
            wrong[name] = (rec, "want kernel %d split %s vendor %s" % (c.kernel, c.split, c.vendor))
    assert not wrong, wrong


def test_every_default_routing_kernel_is_reached_without_a_vendor_route(records):
    # (id 9 needs EDGEDICT_GEMM_NT_TILE=256: out of scope, no entry)
    own = {records[name][0] for name in CASES if records[name][8] == 0}
    assert gemm_cases.DEFAULT_KERNELS - own == set()
    assert 9 not in {r[0] for r in records.values()}


def test_new_entries_never_take_a_vendor_route(records):
    new = [name for name, c in CASES.items() if c.new]
    assert len(new) == 36
    assert [name for name in new if records[name][8] != 0] == []


def test_tn256_entries_cover_edges_item_walk_and_short_last_slice(records):
    tn = [(c, records[c.name]) for c in CASES.values() if records[c.name][0] == 14 and records[c.name][8] == 0]

    def tiles(c):
        return ((c.M + 255) // 256) * ((c.N + 127) // 128)

    assert any(c.M % 256 != 0 for c, r in tn)
    assert any(c.N % 128 != 0 for c, r in tn)
    assert any(r[1] < tiles(c) * r[4] for c, r in tn)               # grid < items: a workgroup walks several
    assert any(r[4] > 1 and c.K % r[5] != 0 for c, r in tn)         # the last K slice is shorter than the others
    assert all(r[7] == 1 for c, r in tn)                            # quiet: the reduce pass follows


def test_every_listed_ragged_tn256_shape_is_there_and_reaches_the_kernel(records):
    # the shapes the kernel's edge clamps, epilogue masks and item walk are checked on (test_gemm_gpu.py): each one on
    # its own - an entry that left, or that plans elsewhere, is noticed here
    for M, N, K, split_k, run in gemm_cases.TN256_RAGGED:
        for form in ("acc", "store"):
            name = "tn256/%dx%dx%d-%s" % (M, N, K, form)
            assert name in CASES, name
            c, rec = CASES[name], records[name]
            assert (c.M, c.N, c.K, c.split_k, c.max_wg, c.margin) == (M, N, K, split_k, 2, True), name
            assert (c.kernel, rec[0], rec[4], rec[8]) == (14, 14, run, 0), (name, rec)
    want = {(4104, 2056, 1031, 1), (264, 1032, 1111, 1), (520, 520, 2100, 4), (1032, 264, 5003, 4), (512, 520, 1024, 8),
            (8, 32768, 1024, 2)}
    assert {t[:4] for t in gemm_cases.TN256_RAGGED} == want
    # what each is there for
    big = records["tn256/4104x2056x1031-acc"]
    assert big[1] < 17 * 17 and (4104 - 8) % 256 == 0 and (2056 - 8) % 128 == 0 and 1031 % 32 != 0
    assert records["tn256/520x520x2100-acc"][4:6] == [4, 576] and (2100 - 3 * 576) % 32 != 0
    assert records["tn256/512x520x1024-acc"][4] == 4
    assert records["tn256/8x32768x1024-acc"][4] == 1
    fb = records["tn256_fallback/1028x264x1031-acc"]
    assert (fb[0], fb[7], fb[8]) == (3, 1, 0)


def test_background_entries_bind_the_residency_cap(records):
    quiet, atomic, two = records["bg/quiet-cap1"], records["bg/atomic-bias-cap1"], records["bg/quiet-cap2"]
    assert (quiet[1], quiet[4], quiet[6], quiet[7]) == (256, 8, 0, 1)       # 512 items on 256 workgroups, reduce pass
    assert (atomic[1], atomic[4], atomic[6], atomic[7]) == (256, 8, 1, 0)   # a bias: atomics into a zeroed C
    assert (two[1], two[4], two[7]) == (512, 8, 1)
    assert records["split/bf16-256x384x4096-bias-store"][6] == 1 and records["split/bf16-130x70x100-clamp"][4] == 2


def test_plan_counts_a_views_offset_and_an_empty_operand(hip_lib):
    import torch
    from edgedict_amd import ops
    full = torch.empty(300, 136, dtype=torch.bfloat16)                # CPU tensors plan as well as meta ones
    b = torch.empty(200, 128, dtype=torch.bfloat16)
    assert ops.gemm_plan(full[:, 8:], b)[0] == 7                      # 16-byte offset: still the direct-to-LDS kernel
    assert ops.gemm_plan(full[:, 4:132], b)[0] == 1                   # 8-byte offset: the guarded generic kernel
    # K = 0: the operands are empty (no address) and C still gets its bias
    a0 = torch.empty(5, 0, device="meta")
    assert ops.gemm_plan(a0, torch.empty(7, 0, device="meta"), bias=torch.empty(7, device="meta"))[0] == 5
