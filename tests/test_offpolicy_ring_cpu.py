"""csrc/erl_common.h erl_ring_refusals / erl_ring_sample_enqueue -- the replay ring's refusals and its interleaved / planar dispatch, shared
by sac_validate / td3_validate and sac_step_layered / td3_step -- checked by a stand-alone host program (tests/offpolicy_ring_main.cpp) under
the address and undefined-behaviour sanitizers: every broken ring alone, one good ring of each kind, the code and the message text the two
validators wrote before they shared the rule.  The program is a child process with no device; nothing is loaded into the interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elegantrl_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "offpolicy_ring_main.cpp")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def build(out, *extra):
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-I", CSRC, *extra, "-o", str(out), MAIN]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_ring_refusals_and_dispatch_under_asan_and_ubsan(tmp_path):
    out = tmp_path / "offpolicy_ring_main"
    r = build(out, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined")
    if r.returncode != 0:            # no sanitizer runtime to link against here: the same program without it
        print("sanitizer build failed, building without it:\n" + r.stdout[-2000:])
        r = build(out)
        assert r.returncode == 0, r.stdout
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "ring ok" in r.stdout and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout
