"""fp16 messages (msg_dtype = f16) where the rest of the suite does not take them: through every form of the column-fused
check kernels, at the edges of the binary16 conversion, and through the hand-over on a staircase code.

fp16 is this repository's own definition, so the expectation is the oracle's msg_f16 mode for plain min-sum and the numpy
restatement for the corrected one (tests/fp16_cases.py; its premises are checked on the CPU in tests/test_fp16_cpu.py).
Everything is compared bit for bit: bytes, iteration counts, all N hard bits, the check->variable messages after two rounds
and the variable->check messages after two rounds.  The last of these is what sees a column-fused kernel that keeps R in a
register at another precision than the one it stores: such an error changes no iteration count and hardly a hard bit
(test_fp16_cpu.py::test_r_kept_unrounded_in_registers_shows_in_the_q_tap_only)."""
import numpy as np
import pytest

import myldpccppapi_amd as L
import fp16_cases as fc
from test_gpu_kernel_matrix import LINK_FORMS

pytestmark = pytest.mark.gpu

FORMS = dict(LINK_FORMS, guided={"link_guided": True})
LINK_KERNELS = {"wide": "check_link_kernel", "narrow": "check_link_narrow_kernel", "half": "check_link_half_kernel"}


def _decoder(c, arith, setting, B, max_iter, V, **kw):
    assert (arith == "msc16") == (setting is not None)
    scale, offset = setting or (0.0, 0.0)
    return L.Decoder(L.Graph(c["rows"], c["cols"], c["M"], c["N"]), c["K"], max_batch=B, algo="ms", msg_dtype="f16",
                     max_iter=max_iter, frames_per_lane=V, ms_scale=scale, ms_offset=offset, **kw)


def _compare(dec, y, want, what):
    """One timed decode and one that stops at the tap: bytes, iteration counts, all N hard bits, R on the frames that
    reached round TAP, Q on those that went on.  Returns the names of the check-phase kernels of the timed decode."""
    B = y.shape[0]
    dec.set_timing(True)
    out, iters = dec.decode(y)
    phase0 = {k["name"] for k in dec.kernel_times() if k["phase"] == 0 and k["name"] != "other"}
    dec.set_timing(False)
    assert np.array_equal(out, want["out"]), ("bytes",) + what
    assert np.array_equal(iters, want["iters"]), ("iterations",) + what
    assert np.array_equal(dec.dump(3, B).astype(np.uint8), want["hard"]), ("hard bits",) + what
    run_r, run_q = fc.tap_frames(want["iters"])
    assert run_q.size > 0, what
    dec.set_tap(fc.TAP)
    dec.decode(y)
    assert fc.same_floats(dec.dump(0, B)[run_r], want["r_tap"][run_r]), ("R tap",) + what
    assert fc.same_floats(dec.dump(1, B)[run_q], want["q_tap"][run_q]), ("Q tap",) + what
    dec.set_tap(0)
    return phase0


def _expected_link_kernel(dec, tune, V):
    """The form the tuning fixes; where it fixes none, V = 1 takes the narrow form and V >= 2 the one timed fastest at
    creation.  The half form has kernels for V = 4 only: below that the launch falls back to the narrow one."""
    if tune.get("link_half"):
        return LINK_KERNELS["half" if V == 4 else "narrow"]
    if "link_narrow" in tune:
        return LINK_KERNELS["narrow" if tune["link_narrow"] else "wide"]
    if tune.get("link_deep") or V == 1:
        return LINK_KERNELS["narrow"]
    lf = dec.link_form()
    assert lf["chosen_by_measurement"] and lf["form"] in (("wide", "narrow", "half") if V == 4 else ("wide", "narrow")), lf
    return LINK_KERNELS[lf["form"]]


@pytest.mark.parametrize("arith", ["ms16", "msc16"])
@pytest.mark.parametrize("d", fc.DEGREES)
def test_fp16_column_fused_forms(built, d, arith):
    """Staircase codes with the linked class at degree d, fp16 messages, plain and corrected min-sum: every form of the
    column-fused check kernel at V = 1, 2, 4 with the unlinked rows riding along in its launch; for d = 7 also with
    launches of their own; and with the fusion off.  By kernel name, the fp16 instantiation of the expected form ran."""
    runs = [("ride", form, tune) for form, tune in FORMS.items()] + [("ride", "unfused", {"link_rows": -1})]
    if d == 7:
        runs.append(("own", "default", {}))
    n = 0
    for kind, form, tune in runs:
        c = fc.staircase(d, kind)
        for V in (1, 2, 4):
            n += 1
            if arith == "ms16":
                settings = (None,)
            else:                # all three on the default form, one of them in turn on the others
                settings = fc.SETTINGS if form == "default" else (fc.SETTINGS[n % 3],)
            for setting in settings:
                what = (d, arith, setting, kind, form, V)
                dec = _decoder(c, arith, setting, fc.FRAMES, fc.MAXIT, V, tune=tune)
                phase0 = _compare(dec, c["y"], fc.want(d, kind, setting), what)
                link = {k for k in phase0 if k.startswith("check_link")}
                if form == "unfused":
                    assert not link and phase0 and all("<%s," % arith in k for k in phase0), (what, phase0)
                else:
                    assert link == {"%s<%s,%d,%d>" % (_expected_link_kernel(dec, tune, V), arith, d, V)}, (what, phase0)
                    if kind == "ride":
                        assert phase0 == link, (what, phase0)
                    else:
                        assert phase0 - link == {"check_group_kernel<%s,1-8,%d>" % (arith, V), "check_kernel<%s,20,%d>" % (arith, V)}, (what, phase0)
                dec.close()


@pytest.mark.parametrize("arith", ["ms16", "msc16"])
@pytest.mark.parametrize("name", ["wimax", "ira"])
def test_fp16_degenerate_channel_values(built, name, arith):
    """Zeros, values that round to binary16's largest number, to infinity and beyond, infinities, NaN, binary16 subnormals
    (the rate matcher's erasure value among them), ties of both grids, -0, and a frame whose Q leaves binary16's range after
    round 1: the stored channel values are the oracle's f16_round of the input, as bits, and everything derived from them is
    what the definition makes of them."""
    c, y = fc.degenerate_code(name), fc.degenerate_inputs(name)
    B = y.shape[0]
    setting = fc.DEGENERATE_SETTING if arith == "msc16" else None
    want = fc.degenerate_want(name, setting is not None)
    stored = fc.f16_round(y)
    for V in (1, 2, 4):
        what = (name, arith, V)
        dec = _decoder(c, arith, setting, B, fc.DEGENERATE_MAXIT, V)
        phase0 = _compare(dec, y, want, what)
        assert phase0 and all("<%s," % arith in k for k in phase0), (what, phase0)
        if name == "ira":
            assert any(k.startswith("check_link") for k in phase0), (what, phase0)
        assert fc.same_floats(dec.dump(2, B), stored), ("channel values",) + what
        dec.close()


def _stats_ok(dec, want, what):
    st = dec.stats()
    assert st["frames_converged"] == want["n_conv"], (what, st)
    assert st["iterations_launched"] == fc.HANDOVER_MAXIT, (what, st)
    return st


def test_fp16_hand_over_on_a_staircase_code(built):
    """fp16 messages on the d = 7 staircase code with 90 scattered stragglers: the host-polled hand-over to child decoders
    (whose linked rows sit elsewhere than the parent's) and the device-side tail, two calls per decoder."""
    import torch
    c = fc.staircase(7, "ride")
    B = fc.HANDOVER_BATCHES[0]
    y = fc.handover_inputs(B)
    runs = [("ms16", None, compact, V) for compact in (512, 7, -1) for V in (1, 4)] + [("msc16", fc.SETTINGS[0], 0, 4)]
    for arith, setting, compact, V in runs:
        want = fc.handover_want(B, setting)
        dec = _decoder(c, arith, setting, B, fc.HANDOVER_MAXIT, V, poll_interval=1, tune={"compact": compact} if compact else {})
        for call in range(2):
            what = ("polled", arith, compact, V, call)
            out, iters = dec.decode(y)
            assert np.array_equal(out, want["out"]), what
            assert np.array_equal(iters, want["iters"]), what
            _stats_ok(dec, want, what)
        dec.close()
    B = fc.HANDOVER_BATCHES[1]
    y, want = fc.handover_inputs(B), fc.handover_want(B)
    yd = torch.from_numpy(y.copy()).cuda()
    nb = L.out_bytes(c["K"], B)
    for tune in ({}, {"compact": 100}, {"device_tail": False}):
        for V in (1, 4):
            dec = _decoder(c, "ms16", None, B, fc.HANDOVER_MAXIT, V, poll_interval=0, tune=tune)
            for call in range(2):
                what = ("device", tune, V, call)
                out = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda")
                it = torch.zeros(B, dtype=torch.int32, device="cuda")
                dec.decode_device(yd.data_ptr(), B, out.data_ptr(), nb, it.data_ptr(), torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy(), want["out"]), what
                assert np.array_equal(it.cpu().numpy(), want["iters"]), what
                assert _stats_ok(dec, want, what)["batch_time"] == fc.HANDOVER_MAXIT, what
            dec.close()
