"""The modem stage without a GPU: ldpc_modem_index against the literal loop of TS 38.212 section 5.4.2.2, ldpc_modem_points
against the formulas of TS 38.211 section 5.1 written out per modulation, the argument checks, and -- with modem_ref and
the oracle alone -- the reference-only facts the GPU tests and DESIGN.md section 8f lean on (every scenario decodes; the
interleaver saves iterations from 16-QAM up)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import myldpccppapi_amd as L
from myldpccppapi_amd import _lib

import modem_ref as mref
import modem_util as MU
import ratematch_util as U

QMS = (1, 2, 4, 6, 8)


def _interleave_38212(E, Qm):
    """f[i + j Qm] = e[i E/Qm + j], the loop as the specification prints it; returns the index of e behind each f."""
    e = np.arange(E, dtype=np.int32)
    f = np.empty(E, np.int32)
    for j in range(E // Qm):
        for i in range(Qm):
            f[i + j * Qm] = e[i * (E // Qm) + j]
    return f


def test_index_equals_the_loop_of_38_212(built):
    for Qm in QMS:
        for S in MU.S_GRID:
            E = S * Qm
            assert np.array_equal(L.Modem(Qm, interleave=True).index(E), _interleave_38212(E, Qm)), (Qm, S)
            assert np.array_equal(L.Modem(Qm, interleave=False).index(E), np.arange(E)), (Qm, S)
            assert np.array_equal(L.Modem(Qm).index(E), _interleave_38212(E, Qm))          # on by default
            for il in (False, True):
                assert np.array_equal(mref.index(Qm, il, E), L.Modem(Qm, interleave=il).index(E))
                assert L.Modem(Qm, interleave=il).symbol_floats(E) == (E if Qm == 1 else 2 * S)


def _points_38211(Qm):
    """d(v) of TS 38.211 section 5.1.2 - 5.1.6 for the label b0 b1 ... (b0 the top bit of v), as complex128."""
    out = np.empty(1 << Qm, np.complex128)
    for v in range(1 << Qm):
        b = [1 - 2 * ((v >> (Qm - 1 - i)) & 1) for i in range(Qm)]          # (1 - 2 b_i)
        if Qm == 1:
            d = b[0]                                                        # the reference's BPSK: real
        elif Qm == 2:
            d = (b[0] + 1j * b[1]) / np.sqrt(2)
        elif Qm == 4:
            d = (b[0] * (2 - b[2]) + 1j * b[1] * (2 - b[3])) / np.sqrt(10)
        elif Qm == 6:
            d = (b[0] * (4 - b[2] * (2 - b[4])) + 1j * b[1] * (4 - b[3] * (2 - b[5]))) / np.sqrt(42)
        else:
            d = (b[0] * (8 - b[2] * (4 - b[4] * (2 - b[6]))) + 1j * b[1] * (8 - b[3] * (4 - b[5] * (2 - b[7])))) / np.sqrt(170)
        out[v] = d
    return out


@pytest.mark.parametrize("Qm", QMS)
def test_points_equal_the_formulas_of_38_211(built, Qm):
    got = L.Modem(Qm).points()
    assert got.dtype == np.float32 and got.shape == (1 << Qm, 2)
    want = _points_38211(Qm)
    assert np.abs(got[:, 0] - want.real).max() < 1e-7 and np.abs(got[:, 1] - want.imag).max() < 1e-7
    assert np.array_equal(got.view(np.uint32), mref.points(Qm).view(np.uint32))
    assert abs(float((got.astype(np.float64) ** 2).sum(axis=1).mean()) - 1.0) < 1e-6
    if Qm >= 2:
        # per axis: exactly the odd integers in +-(2^m - 1) times A, and neighbouring levels differ in one bit
        m = Qm // 2
        lab, lev = mref.axis_levels(Qm)
        order = np.argsort(lev)
        assert np.array_equal(np.rint(lev[order].astype(np.float64) * np.sqrt(mref.NORM[Qm])), np.arange(-(2 ** m - 1), 2 ** m, 2))
        assert ((lab[order][1:] != lab[order][:-1]).sum(axis=1) == 1).all()
        assert set(np.unique(got[:, 0])) == set(lev) and set(np.unique(got[:, 1])) == set(lev)


def _spec(Qm=4, interleave=1):
    lib = _lib.load()
    s = _lib.ModemSpec()
    lib.ldpc_modem_spec_init(ctypes.byref(s), Qm)
    assert s.struct_size == ctypes.sizeof(_lib.ModemSpec) == 12 and s.Qm == Qm and s.interleave == int(Qm >= 2)
    s.interleave = interleave
    return s


def test_argument_errors_name_the_field(built):
    """Every refusal is judged before a device is touched: the pointers here are never dereferenced."""
    lib = _lib.load()
    p, q = 1 << 20, 1 << 24
    ok = _spec()

    def transmit(spec=ok, tx=p, fmt=1, frames=4, E=64, sd=0.3, first=0, sym=q, cap=1 << 20):
        return lib.ldpc_modem_transmit_device(ctypes.byref(spec), tx, fmt, frames, E, sd, 7, first, sym, cap, 0, None)

    def demap(spec=ok, sym=p, frames=4, E=64, rx=q):
        return lib.ldpc_modem_demap_device(ctypes.byref(spec), sym, frames, E, rx, 0, None)

    bad_size = _spec()
    bad_size.struct_size -= 4
    for call, word in ((lambda: transmit(spec=_spec(3)), "Qm"), (lambda: demap(spec=_spec(3)), "Qm"), (lambda: transmit(spec=_spec(0)), "Qm"),
                       (lambda: transmit(E=66), "E % Qm"), (lambda: demap(E=66), "E % Qm"), (lambda: transmit(E=0), "E"),
                       (lambda: transmit(fmt=0, E=60), "E % 8"), (lambda: transmit(fmt=5), "tx_format"),
                       (lambda: transmit(sd=-0.1), "sd"), (lambda: transmit(sd=float("nan")), "sd"), (lambda: transmit(sd=float("inf")), "sd"),
                       (lambda: transmit(cap=4 * 32 - 1), "sym_floats"), (lambda: transmit(spec=_spec(1, 0), cap=4 * 64 - 1), "sym_floats"),
                       (lambda: transmit(frames=-1), "frames"), (lambda: demap(frames=-1), "frames"), (lambda: transmit(first=-1), "first_frame"),
                       (lambda: transmit(tx=None), "NULL"), (lambda: demap(rx=None), "NULL"),
                       (lambda: demap(rx=p), "overlap"), (lambda: demap(rx=p + 4 * 4 * 32 - 4), "overlap"), (lambda: demap(sym=q + 4 * 4 * 64 - 4), "overlap"),
                       (lambda: transmit(sym=p + 4 * 64 - 4), "overlap"),
                       (lambda: transmit(spec=bad_size), "struct_size"), (lambda: demap(spec=bad_size), "struct_size"),
                       (lambda: transmit(spec=_spec(4, 2)), "interleave")):
        assert call() == 1, word
        assert word in lib.ldpc_last_error().decode(), (word, lib.ldpc_last_error().decode())
    out = np.zeros(64, np.int32)
    assert lib.ldpc_modem_index(ctypes.byref(bad_size), 64, out.ctypes.data) == 1 and "struct_size" in lib.ldpc_last_error().decode()
    assert lib.ldpc_modem_index(ctypes.byref(ok), 66, out.ctypes.data) == 1 and "E % Qm" in lib.ldpc_last_error().decode()
    assert lib.ldpc_modem_index(None, 64, out.ctypes.data) == 1
    assert lib.ldpc_modem_points(3, out.ctypes.data) == 1 and "Qm" in lib.ldpc_last_error().decode()
    assert lib.ldpc_modem_symbol_floats(ctypes.byref(ok), 66) == 0 and lib.ldpc_modem_symbol_floats(ctypes.byref(ok), 64) == 32
    with pytest.raises(L.LdpcError) as e:
        L.Modem(3)
    assert e.value.code == 1
    # adjacent buffers and frames == 0 are fine (frames == 0 enqueues nothing and touches no device)
    assert demap(frames=0) == 0 and transmit(frames=0, cap=0) == 0


def test_compute_entry_points_have_no_cpu_path(built):
    """Host buffers: without a device LDPC_ERR_HIP, with one the call simply runs."""
    md = L.Modem(4)
    tx = np.zeros((2, 64), np.uint8)
    if L.device_count() > 0:
        assert md.demap(md.transmit(tx, 0.0, 1), 64).shape == (2, 64)
        return
    with pytest.raises(L.LdpcError) as e:
        md.transmit(tx, 0.3, 1)
    assert e.value.code == 2
    with pytest.raises(L.LdpcError) as e:
        md.demap(np.zeros((2, 32), np.float32), 64)
    assert e.value.code == 2
    lib = _lib.load()
    s = _spec()
    assert lib.ldpc_modem_transmit_device(ctypes.byref(s), 1 << 20, 1, 4, 64, 0.3, 7, 0, 1 << 24, 1 << 20, 0, None) == 2
    assert lib.ldpc_modem_demap_device(ctypes.byref(s), 1 << 20, 4, 64, 1 << 24, 0, None) == 2


def test_coder_exports_set_modulation(built):
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myldpccppapi_amd", "libmyldpc.so")
    syms = subprocess.run("nm -D --defined-only %s | c++filt" % so, shell=True, capture_output=True, text=True).stdout
    assert "Coder::setModulation(int, bool)" in syms


def test_coder_without_set_modulation_is_the_reference_channel(built, tmp_path):
    """tests/cpp/coder_modulation.cpp, the parts that need no device: test() without setModulation writes the reference's
    BPSK + gaussian() samples bit for bit; setModulation refuses Qm = 3 and bits per frame that do not fill symbols."""
    out = subprocess.run([MU.coder_modulation_exe(tmp_path), "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "refused=ok plain=ok" in out.stdout, out.stdout + out.stderr


# ---- modem_ref and the oracle alone: entries of the table in DESIGN.md section 8f ----------------------------------

@pytest.mark.parametrize("Qm", QMS)
def test_noiseless_demap_has_the_sign_of_every_bit(Qm):
    rng = np.random.default_rng(50 + Qm)
    for il in (False, True):
        for S in MU.S_GRID:
            E = S * Qm
            bits = rng.integers(0, 2, (3, E), dtype=np.uint8)
            y = mref.demap(Qm, il, mref.transmit(Qm, il, bits, 0.0, 1, 0, None), E)
            assert y.dtype == np.float32 and (y != 0).all() and np.array_equal(y < 0, bits != 0), (Qm, il, S)


def test_bpsk_transmit_is_the_channel_of_ldpc_awgn():
    import oracle
    bits = np.random.default_rng(56).integers(0, 2, (3, 37), dtype=np.uint8)
    got = mref.transmit(1, False, bits, 0.7, 9, 2 ** 32 + 5, MU.chlib())
    assert np.array_equal(got.view(np.uint32), oracle.awgn(37, 2 ** 32 + 5, 3, 0.7, seed=9, codewords=bits).view(np.uint32))


@pytest.mark.parametrize("Qm", sorted(MU.POINTS))
def test_every_scenario_decodes_and_the_interleaver_saves_iterations(Qm):
    mean = {}
    for il in (True, False):
        for algo in ("layered", "ms", "sp"):
            _, iters, wrong = MU.oracle_decode(Qm, il, algo)
            mean[il, algo] = float(np.mean(iters))
            print("Qm %d sd %.2f raw BER %.3f %-7s interleave %d: %d / %d frames wrong, mean iterations %.2f"
                  % (Qm, MU.POINTS[Qm], MU.raw_ber(Qm, il), algo, il, wrong, U.FRAMES, mean[il, algo]))
            assert wrong == 0, (Qm, il, algo)
    if Qm >= 4:
        for algo in ("layered", "ms", "sp"):
            assert mean[True, algo] <= mean[False, algo], (Qm, algo, mean)


def test_sum_product_needs_the_matched_scale_at_64_qam():
    """The reference's constant llr_scale = 8 fails every frame at 64-QAM, sd 0.2; 2 / sd^2 = 50 decodes them all."""
    import oracle
    r = oracle.decode(U.bg1()[2], MU.recovered(6, True, 10.0), "sp", max_iter=U.MAX_ITER, llr_scale=8.0, layer_rows=U.Z)
    wrong = (np.asarray(r["out"]).reshape(U.FRAMES, U.K // 8) != U.payload()[1].reshape(U.FRAMES, U.K // 8)).any(axis=1)
    assert int(wrong.sum()) == U.FRAMES
    assert MU.oracle_decode(6, True, "sp")[2] == 0
    # the matched scale stays below the fp32 exp limit on these inputs
    for Qm, sd in MU.POINTS.items():
        scale, fill = MU.matched_scale(sd)
        assert scale * float(np.abs(MU.recovered(Qm, True, fill)).max()) < 88.0, Qm
