"""Decoder configuration without a GPU: csrc/decoder_config_host.hpp under the host sanitizers, and every refusal
ldpc_decoder_create makes in front of the device check against the answers recorded before validation moved into that
header (decoder_config_cases.py says how)."""
import os
import subprocess

import numpy as np

from myldpccppapi_amd import _lib

import decoder_config_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_header_under_host_sanitizers(tmp_path):
    """The header in a stand-alone program built with the address and undefined-behaviour sanitizers: the algorithm table,
    config_in on every size, pick_frames_per_lane at its thresholds, engine_candidates of every creation branch."""
    exe = str(tmp_path / "decoder_config_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "decoder_config_host_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr


def test_refusals_are_what_they_were(built):
    """Code and message of every case of the sweep, byte for byte; a case that passed validation still does and stops at
    the device check."""
    want = np.load(os.path.join(ROOT, "tests", "golden", "decoder_config_refusals.npz"))
    names = [name for name, _ in DC.cases()]
    assert str(want["names_sha256"]) == DC.names_sha256() and len(names) == want["code"].size == want["index"].size
    messages = [str(m) for m in want["messages"]]
    got = DC.answers(_lib.load(), DC.graph())
    assert len(got) == len(names)
    wrong = []
    for name, (code, msg), wcode, windex in zip(names, got, want["code"].tolist(), want["index"].tolist()):
        wmsg = None if windex < 0 else messages[windex]
        if (code, msg) != (wcode, wmsg):
            wrong.append((name, (code, msg), (wcode, wmsg)))
    print("%d cases, %d passed validation, %d differ" % (len(got), sum(m is None for _, m in got), len(wrong)))
    assert not wrong, wrong[:5]
    # the sweep is not vacuous: it reaches the device check and both refusal codes, from every kind of rule
    assert sum(i < 0 for i in want["index"].tolist()) > 1000 and len(messages) >= 100
    assert set(want["code"].tolist()) == {1, 2, 4}
