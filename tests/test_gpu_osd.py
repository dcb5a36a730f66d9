"""Ordered-statistics decoding on the GPU (ldpc_osd_device / ldpc_osd_run, L.Osd, Coder::setOsd) against osd_ref,
exactly: code, out, status and metric as integers.  Behind a min-sum and a BP decoder, on synthetic rows (ties, zeros, NaN,
inf, the cap, all clean, all dirty), on hard decisions with crafted syndromes (rows that one lane of the flag pass
owns together), on every shape class of the rule, on shifted pointers with guard regions around every
output, each output alone, a stream of its own, two calls on one handle, the host form across chunks, the refusals."""
import numpy as np
import pytest

import myldpccppapi_amd as L

import osd_cases as OC
import osd_ref

pytestmark = pytest.mark.gpu

GUARD, MARK = 64, 0xEE
ALL = ("out", "code", "status", "metric")


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def handles(built):
    made = {}

    def get(name, max_frames=128):
        if (name, max_frames) not in made:
            c = OC.code(name)
            g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
            made[(name, max_frames)] = (g, L.Osd(g, c["K"], max_frames=max_frames))
        return made[(name, max_frames)][1]
    yield get
    for g, o in made.values():
        o.close()
        g.close()


def _buf(nbytes, shift):
    """A marker-filled device buffer of nbytes bytes with GUARD + shift marker bytes in front and GUARD behind."""
    t = _torch().full((GUARD + shift + nbytes + GUARD,), MARK, dtype=_torch().uint8, device="cuda")
    return t, t.data_ptr() + GUARD + shift


def _down(t, nbytes, shift, what, dtype=np.uint8):
    host = t.cpu().numpy()
    lo = GUARD + shift
    assert (host[:lo] == MARK).all() and (host[lo + nbytes:] == MARK).all(), "wrote outside the %s buffer" % what
    return host[lo:lo + nbytes].copy().view(dtype)


def run_device(osd, soft, order, scale, outputs=ALL, byte_shift=0, word_shift=0, stream=None):
    """dict of the outputs asked for; soft sits word_shift bytes (a multiple of 4) behind an aligned address, byte outputs
    byte_shift bytes, int32 outputs word_shift bytes."""
    torch = _torch()
    soft = np.ascontiguousarray(soft, np.float32).reshape(-1, osd.N)
    frames, nb = soft.shape[0], osd.K // 8
    src = torch.zeros(word_shift + soft.size * 4 + 4, dtype=torch.uint8, device="cuda")
    if soft.size:
        src[word_shift:word_shift + soft.size * 4] = torch.from_numpy(soft.reshape(-1).view(np.uint8).copy()).cuda()
    sizes = {"out": frames * nb, "code": frames * osd.N, "status": frames * 4, "metric": frames * 4}
    shifts = {"out": byte_shift, "code": byte_shift, "status": word_shift, "metric": word_shift}
    bufs = {k: _buf(sizes[k], shifts[k]) for k in outputs}
    ptr = {k: (bufs[k][1] if k in bufs else None) for k in ALL}
    osd.run_device(src.data_ptr() + word_shift, frames, order, scale, ptr["out"], sizes["out"] if "out" in bufs else 0, ptr["code"],
                   ptr["status"], ptr["metric"], _stream() if stream is None else stream)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy()[word_shift:word_shift + soft.size * 4].view(np.float32).view(np.uint32),
                          soft.reshape(-1).view(np.uint32)), "the input was changed"
    got = {}
    for k in outputs:
        a = _down(bufs[k][0], sizes[k], shifts[k], k, np.int32 if k in ("status", "metric") else np.uint8)
        got[k] = a.reshape(frames, nb if k == "out" else osd.N) if k in ("out", "code") else a
    return got


def check(got, want, what):
    for k, v in got.items():
        w = want[k].reshape(v.shape)
        assert np.array_equal(v, w), "%s: %s differs from the reference in frames %s" % (
            what, k, np.flatnonzero((v != w).reshape(v.shape[0], -1).any(axis=1))[:8])


def reference(name, soft, order, scale):
    c = OC.code(name)
    return osd_ref.run(c["H"], soft, order, scale, c["K"])


# ---- behind a decoder ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo", ["ms", "bp"])
def test_decoder_chain(handles, algo):
    """96 frames of (576, 288): ldpc_decode_soft_device -> ldpc_osd_device in HBM, orders 0 and 1; the soft values are those
    of the reference's decoder, bit for bit, so the premises test_osd_cpu.py checks hold for what the kernel sees."""
    torch = _torch()
    c, y = OC.code(OC.WIMAX_HALF), OC.decoder_y()
    frames, N, K = y.shape[0], c["N"], c["K"]
    osd = handles(OC.WIMAX_HALF)
    dec = L.Decoder(osd.graph, K, max_batch=frames, algo=algo, max_iter=OC.DECODER_MAXIT, llr_scale=OC.BP_LLR_SCALE if algo == "bp" else 8.0)
    llr = torch.from_numpy(np.array(y)).cuda()
    soft = torch.zeros((frames, N), dtype=torch.float32, device="cuda")
    dec_out = torch.zeros(frames * K // 8, dtype=torch.uint8, device="cuda")
    for order in (0, 1):
        out = torch.full((frames, K // 8), MARK, dtype=torch.uint8, device="cuda")
        code = torch.full((frames, N), MARK, dtype=torch.uint8, device="cuda")
        status = torch.full((frames,), -77, dtype=torch.int32, device="cuda")
        metric = torch.full((frames,), -77, dtype=torch.int32, device="cuda")
        dec.decode_device(llr.data_ptr(), frames, dec_out.data_ptr(), dec_out.numel(), None, _stream(), soft_ptr=soft.data_ptr(),
                          soft_floats=soft.numel())
        osd.run_device(soft.data_ptr(), frames, order, OC.SCALE, out.data_ptr(), out.numel(), code.data_ptr(), status.data_ptr(),
                       metric.data_ptr(), _stream())
        torch.cuda.synchronize()
        post = soft.cpu().numpy()
        assert np.array_equal(post.view(np.uint32), OC.decoder_post(algo).view(np.uint32)), "the decoder's posterior is not the reference's"
        want = reference(OC.WIMAX_HALF, post, order, OC.SCALE)
        got = dict(out=out.cpu().numpy(), code=code.cpu().numpy(), status=status.cpu().numpy(), metric=metric.cpu().numpy())
        print(algo, "order", order, "status counts", np.bincount(got["status"], minlength=3), "frames still wrong", int(got["code"].any(axis=1).sum()))
        check(got, want, (algo, order))
        clean = got["status"] == 0
        assert np.array_equal(got["out"][clean], dec_out.cpu().numpy().reshape(frames, -1)[clean]), "a clean frame's bytes are not the decoder's"
    dec.close()


# ---- synthetic rows -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ties", "specials", "all_clean", "all_dirty"])
def test_synthetic_rows(handles, kind):
    soft, scale = OC.synthetic(kind)
    osd = handles(OC.WIMAX_HALF)
    for order in (0, 1):
        got = run_device(osd, soft, order, scale)
        print(kind, "order", order, "status counts", np.bincount(got["status"], minlength=3))
        check(got, OC.want(OC.WIMAX_HALF, kind, order), (kind, order))


@pytest.mark.parametrize("name", sorted(OC.CRAFTED))
def test_crafted_syndromes(handles, name):
    """Hard decisions whose unsatisfied checks are exactly rows m and m + 256 (+ 512): the flag pass must not let the
    parities of the rows one lane owns cancel; and a single unsatisfied row beyond row 255."""
    soft, sets = OC.crafted(name)
    osd = handles(name)
    for order in (0, 1):
        got = run_device(osd, soft, order, OC.SCALE)
        print(name, "order", order, "status", list(got["status"]))
        assert (got["status"] > 0).all(), "a dirty frame was taken for clean: %s" % [sets[f] for f in np.flatnonzero(got["status"] == 0)]
        check(got, OC.crafted_want(name, order), (name, order))


# ---- shapes ---------------------------------------------------------------------------------------------------------------

SHAPES = [("n100", 12), ("deficient", 12), ("hamming", 16), ("bg1", 8), (OC.WIMAX_LONG, 6), (OC.WIMAX_HIGH, 6)]


@pytest.mark.parametrize("name,frames", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes(handles, name, frames):
    """N no multiple of 32, a rank-deficient H, a code of one word per row, 34 words per row with 736 rows (BG1-profile:
    the largest LDS footprint among the named codes, 116 952 bytes), 36 words per row (98 672 bytes), a high-rate code"""
    c = OC.code(name)
    osd = handles(name)
    info = osd.info()
    assert (info["M"], info["N"], info["words_per_row"]) == (c["M"], c["N"], (c["N"] + 31) // 32) and info["lds_bytes"] <= 160 * 1024 - 512
    soft = OC.shape_rows(name, frames, seed=len(name))
    for order in (0, 1):
        want = reference(name, soft, order, OC.SCALE)
        print(name, "order", order, "status counts", np.bincount(want["status"], minlength=3), "lds", info["lds_bytes"])
        assert (want["status"] > 0).sum() >= 3
        got = run_device(osd, soft, order, OC.SCALE, outputs=ALL if c["K"] % 8 == 0 else ALL[1:])
        check(got, want, (name, order))


# ---- calling conventions ------------------------------------------------------------------------------------------------

def test_frame_counts_offsets_and_single_outputs(handles):
    soft, scale = OC.synthetic("specials")
    want = OC.want(OC.WIMAX_HALF, "specials", 1)
    osd = handles(OC.WIMAX_HALF, 24)
    for frames in (0, 1, 24):                                   # 24 = max_frames
        for byte_shift, word_shift in ((0, 0), (1, 4), (3, 12)):
            got = run_device(osd, soft[:frames], 1, scale, byte_shift=byte_shift, word_shift=word_shift)
            check(got, {k: want[k][:frames] for k in ALL}, (frames, byte_shift, word_shift))
    for k in ALL:                                               # every output alone, the others NULL
        got = run_device(osd, soft, 1, scale, outputs=(k,), byte_shift=1, word_shift=4)
        check(got, want, ("alone", k))


def test_stream_of_its_own_and_two_calls_on_one_handle(handles):
    torch = _torch()
    osd = handles(OC.WIMAX_HALF)
    a, sa = OC.synthetic("all_dirty")
    b, sb = OC.synthetic("specials")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got_a = run_device(osd, a, 1, sa, stream=s.cuda_stream)
        got_b = run_device(osd, b, 0, sb, stream=s.cuda_stream)
        got_a2 = run_device(osd, a, 1, sa, stream=s.cuda_stream)
    check(got_a, OC.want(OC.WIMAX_HALF, "all_dirty", 1), "first call")
    check(got_b, OC.want(OC.WIMAX_HALF, "specials", 0), "second call")
    check(got_a2, OC.want(OC.WIMAX_HALF, "all_dirty", 1), "third call")


def test_host_form_across_chunks(handles):
    """ldpc_osd_run: 24 frames through a handle of max_frames = 7 -- chunks of 7, 7, 7, 3"""
    soft, scale = OC.synthetic("specials")
    c = OC.code(OC.WIMAX_HALF)
    g = L.Graph(c["rows"], c["cols"], c["M"], c["N"])
    osd = L.Osd(g, c["K"], max_frames=7)
    for order in (0, 1):
        out, code, status, metric = osd.run(soft, order, scale)
        check(dict(out=out, code=code, status=status, metric=metric), OC.want(OC.WIMAX_HALF, "specials", order), ("host", order))
    osd.close()


def test_refusals_that_need_a_device(handles):
    torch = _torch()
    osd = handles(OC.WIMAX_HALF, 24)
    N, K = osd.N, osd.K
    soft = torch.zeros(24 * N + 8, dtype=torch.float32, device="cuda")
    out = torch.full((24 * K // 8 + 8,), MARK, dtype=torch.uint8, device="cuda")
    st = torch.full((32,), -77, dtype=torch.int32, device="cuda")

    def refused(code, needle, *a, **kw):
        with pytest.raises(L.LdpcError) as e:
            osd.run_device(*a, **kw)
        assert e.value.code == code and needle in str(e.value), str(e.value)

    refused(1, "order", soft.data_ptr(), 4, 2, 256.0, out.data_ptr(), out.numel())
    refused(1, "weight_scale", soft.data_ptr(), 4, 1, 0.0, out.data_ptr(), out.numel())
    refused(1, "weight_scale", soft.data_ptr(), 4, 1, float("nan"), out.data_ptr(), out.numel())
    refused(1, "max_frames", soft.data_ptr(), 25, 1, 256.0, out.data_ptr(), out.numel())
    refused(1, "out_bytes", soft.data_ptr(), 4, 1, 256.0, out.data_ptr(), 4 * K // 8 - 1)
    refused(1, "NULL", soft.data_ptr(), 4, 1, 256.0)
    refused(1, "aligned", soft.data_ptr() + 2, 4, 1, 256.0, out.data_ptr(), out.numel())
    refused(1, "aligned", soft.data_ptr(), 4, 1, 256.0, None, 0, None, st.data_ptr() + 1)
    refused(1, "overlaps", soft.data_ptr(), 4, 1, 256.0, None, 0, soft.data_ptr() + 4 * N)             # code inside soft
    refused(1, "overlaps", soft.data_ptr(), 4, 1, 256.0, None, 0, None, soft.data_ptr() + 16 * N - 4)   # status on soft's last word
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == MARK).all() and (st.cpu().numpy() == -77).all(), "a refused call wrote"
    with pytest.raises(L.LdpcError) as e:
        c = OC.code(OC.WIMAX_HALF)
        L.Osd(osd.graph, c["K"], device=4096)
    assert e.value.code == 1 and "device" in str(e.value)


# ---- Coder --------------------------------------------------------------------------------------------------------------

def test_coder_set_osd(built, tmp_path):
    """tests/cpp/coder_osd.cpp: the bytes of Coder::decode with setOsd(1) equal those of the C ABI chain and the reference's"""
    import coder_osd_harness as H
    H.run_gpu(tmp_path)
