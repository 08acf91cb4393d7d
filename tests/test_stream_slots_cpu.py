"""csrc/stream_slots.h -- the one (device, stream) table behind every library-owned buffer, and its one grow rule -- checked by a
stand-alone host program (tests/stream_slots_main.cpp): claim / find / exhaustion / release, a failed grow (no device is needed: without one
hipMalloc fails cleanly), and the table's lock under eight threads with the thread sanitizer.  The program is a child process; nothing
is loaded into the interpreter."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "elegantrl_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "stream_slots_main.cpp")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def build(out, *extra):
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-I", CSRC, *extra, "-o", str(out), MAIN, "-lpthread"]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def run(exe, case):
    # no device for the child: the failed-grow case is about an allocation that fails
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([str(exe), case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=120)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("stream_slots") / "stream_slots_main"
    r = build(out)
    assert r.returncode == 0, r.stdout
    return out


def test_claim_find_exhaustion_release_and_failed_grow(exe):
    """the failed-grow half is the regression test of the two defects of the hand-written caches (a slot whose regrow failed kept
    its old size and looked free, with its second buffer still attached): the entry stays with its key, buffer null and size 0"""
    r = run(exe, "table")
    assert r.returncode == 0 and "table ok" in r.stdout, r.stdout


def test_eight_threads_under_the_thread_sanitizer(tmp_path):
    out = tmp_path / "stream_slots_tsan"
    r = build(out, "-Xarch_host", "-fsanitize=thread")
    if r.returncode != 0:            # no sanitizer runtime to link against here: the same case without it
        print("thread sanitizer build failed, building without it:\n" + r.stdout[-2000:])
        r = build(out)
        assert r.returncode == 0, r.stdout
    r = run(out, "threads")
    assert r.returncode == 0 and "threads ok" in r.stdout and "ThreadSanitizer" not in r.stdout, r.stdout
