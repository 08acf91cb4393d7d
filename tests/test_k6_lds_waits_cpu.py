"""The split-arithmetic minibatch kernel's LDS waits, as a build-time check (tools/k6_lds_wait_sites.py): in the [128,128] instantiations
no full `s_waitcnt lgkmcnt(0)` stands directly behind a batch of transposing reads whose registers the next MFMA group does not read
(54 such sites before the phase stamps went through an LDS-typed pointer), none behind a ds_bpermute whose result
the next instruction is not the first to need, and every ds_read_b128 site that remains is one DESIGN.md names.  Compiles one
translation unit to assembly (hipcc cross-compiles without a GPU; ~45 s)."""
import io
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def sites():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import k6_lds_wait_sites as T
    path = T.compile_unit("ppo_step_s3_pre.hip", [])
    try:
        text = io.StringIO()
        res = T.report(path, list_sites=True, out=text)
    finally:
        os.unlink(path)
    print(text.getvalue())
    return T, res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_no_full_wait_behind_reads_not_yet_needed(sites):
    T, res = sites
    kernels = [k for k in res if "ppo_step_s3_kernelILi" in k and "ELi4ELi4E" in k]
    assert len(kernels) == 5, kernels                                     # S <= 8, S <= 32 and S <= 64, rows aligned or not
    for k in kernels:
        assert set(res[k]) == {"actor", "critic"}, (k, list(res[k]))
        assert T.unneeded(res, k, "ds_read_b64_tr_b16") == 0, k
        for path, ss in res[k].items():
            hops = [s for s in ss if s["kind"] == "ds_bpermute" and not s["immediate"]]
            assert not hops, (k, path, hops)
        # DESIGN.md section 4 names no remaining unneeded ds_read_b128 site: there is none
        assert T.unneeded(res, k, "ds_read_b128") == 0, k


def test_the_tool_finds_the_sites_of_a_known_listing(tmp_path):
    """the classifier on a hand-written listing: an unneeded site (the wait guards the OTHER buffer), a needed one, a barrier guard"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import k6_lds_wait_sites as T
    mf = "\tv_mfma_f32_32x32x16_bf16 v[18:33], v[100:103], {b}, v[18:33]\n"
    asm = ("_ZN1_18ppo_step_s3_kernelILi2ELi4ELi4ELb1ELb1EEEv8Ppo2Args:\n"
           "\tds_read_b64_tr_b16 v[14:15], v59\n\tds_read_b64_tr_b16 v[16:17], v60\n\ts_waitcnt lgkmcnt(0)\n" + mf.format(b="v[2:5]") * 6
           + "\tds_read_b64_tr_b16 v[2:3], v59\n\tds_read_b64_tr_b16 v[4:5], v60\n\ts_waitcnt lgkmcnt(0)\n" + mf.format(b="v[2:5]") * 6
           + "\tds_read_b128 v[40:43], v1\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n"
           + "\tds_bpermute_b32 v7, v8, v9\n\ts_waitcnt lgkmcnt(0)\n\tv_mov_b32_e32 v1, v2\n\tv_add_f32_e32 v9, v9, v7\n\ts_endpgm\n.Lfunc_end0:\n")
    p = tmp_path / "k.s"
    p.write_text(asm)
    res = T.report(str(p), out=io.StringIO())
    (ss,) = [v for ps in res.values() for v in ps.values()]
    assert [(s["kind"], s["needed"], s["immediate"]) for s in ss] == [("ds_read_b64_tr_b16", False, False), ("ds_read_b64_tr_b16", True, True),
                                                                       ("ds_read_b128", True, True), ("ds_bpermute", True, False)]
