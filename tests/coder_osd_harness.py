"""Builds tests/cpp/coder_osd.cpp (Coder::setOsd end to end) against the in-tree libraries and holds what it writes
against osd_ref."""
import os
import subprocess

import numpy as np

import osd_cases as OC
import osd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def coder_osd_exe(tmp_path):
    exe = str(tmp_path / "coder_osd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "coder_osd.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "myldpccppapi_amd"), "-lmyldpc", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myldpccppapi_amd")])
    return exe


def run_host(tmp_path):
    """the parts that need no device"""
    out = subprocess.run([coder_osd_exe(tmp_path), "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "refused=ok", out.stdout + out.stderr


def run_gpu(tmp_path):
    out = subprocess.run([coder_osd_exe(tmp_path), str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(out.stdout.strip())
    assert out.returncode == 0, out.stdout + out.stderr
    fields = dict(f.split("=") for f in out.stdout.split())
    assert fields["refused"] == "ok" and fields["same"] == "ok" and fields["counts"] == "ok", out.stdout
    c = OC.code(OC.WIMAX_HALF)
    post = np.fromfile(str(tmp_path / "post.f32"), np.float32).reshape(-1, c["N"])
    want = osd_ref.run(c["H"], post, 1, 256.0, c["K"])
    assert np.array_equal(np.fromfile(str(tmp_path / "coder.u8"), np.uint8), want["out"].reshape(-1))
    assert np.array_equal(np.fromfile(str(tmp_path / "chain.u8"), np.uint8), want["out"].reshape(-1))
    assert np.array_equal(np.fromfile(str(tmp_path / "status.i32"), np.int32), want["status"])
    # the case is worth its time: frames of every status, and fewer wrong frames behind the stage than in front of it
    assert min(np.bincount(want["status"], minlength=3)) >= 3 and int(fields["after"]) < int(fields["before"]), out.stdout
