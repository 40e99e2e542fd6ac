"""The fp32 frame of an evaluation - the conditioning chain (k_time_features, k_time_features_steps, k_dense_rows, k_dense_tiled,
k_dense_mfma), the two embeddings (k_embed in its register forms, k_embed_mfma), k_ln_inplace, the k_embed<STATS> + k_ln_finalize pair of
ln_fuse handles and the output head fused with the sampler's update (k_head_step_mfma) - element by element against fp64 references built
from the very fp32 operands the kernels read (lsl_debug_mods_ex, lsl_debug_mods_steps, lsl_debug_embed, lsl_debug_head), at the case
tables of frame_cases.py.

Every element of every tensor must lie within its bar (derivation: frame_cases.py; u = 2^-24):
  * tfeat                 K_TRIG u against cos / sin in fp64 of the kernel's fp32 argument
  * hid, vec, mods, yhid, yemb   (K + 3) u sum|w x| + u per added term, the silu terms in front of / behind the chain
  * cond_emb, h           (C + 3) u sum|w x| + u per added term
  * hn (normalize)        the LayerNorm statistics term; stats (ln_fuse): relative bars of rstd and -mean rstd
  * head out              the LayerNorm + modulate error through sum|Wo| + (D + 3) u sum|Wo a|; state update: |am| bar(m) + 4 u sum|terms|
conftest.parity prints the worst element of each (case, tensor) in units of its bar; the record is profiles/frame_rowwise_parity.txt.
Bit equalities where the library promises bits: trace / save_out, device noise against the library's own draw, lsl_debug_mods against
lsl_debug_mods_ex, the rows of lsl_debug_mods_steps against the single-row calls, the STATS embedding against the plain one, a shared
modulation row against identical rows, repeated calls of the multi-tile cases.

A comparison counts only for the kernel it names: the library's own labels (lsl_profile_kernel_name, classes 4, 5 and 6) must be the ones
frame_cases derives for 256 CUs, so a device with another CU count fails loudly instead of testing another form."""
import ctypes as C
import time

import pytest
import torch

import frame_cases as fc
from conftest import parity
from test_hip_parity import build_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    # the tile-to-workgroup maps test_frame_cases.py proves are those of fc.CUS compute units; not every label names the grid
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == fc.CUS, f"the case tables are laid out for {fc.CUS} CUs, this device has {cus}"
    return torch.device("cuda:0")


_NETS = {}
_WEIGHTS = {}


def _net(C_, D, V, normalize, lnf, dev):
    key = (C_, D, V, normalize, lnf)
    if key not in _NETS:
        if len(_NETS) >= 6:  # (a handful of handles at a time: the large cases bring large scratch buffers)
            _NETS.pop(next(iter(_NETS)))
        sh, p = fc.params(C_, D, V, normalize)
        net = build_net(sh, p, dev)
        if lnf:
            net.set_ln_fuse(True)
        net.ensure_packed(dev)
        assert net.ln_fuse == bool(lnf)
        _NETS[key] = net
    return _NETS[key]


def _weights(C_, D, V, normalize, dev):
    key = (C_, D, V, normalize)
    if key not in _WEIGHTS:
        if len(_WEIGHTS) >= 4:
            _WEIGHTS.pop(next(iter(_WEIGHTS)))
        _WEIGHTS[key] = fc.frame_weights(fc.params(C_, D, V, normalize)[1], dev)
    return _WEIGHTS[key]


def _lib():
    from lam_slide_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _labelled(net, cls, call):
    """call() with profile class cls bracketed: the label the library's own dispatch left."""
    L, lib = _lib()
    L.check(lib.lsl_profile_enable(net._handle, cls, 8))
    try:
        call()
        torch.cuda.synchronize()
        return lib.lsl_profile_kernel_name(net._handle).decode()
    finally:
        lib.lsl_profile_enable(net._handle, -1, 0)


def _ws(net, B, T, L_, dev):
    _, lib = _lib()
    return torch.empty(int(lib.lsl_workspace_bytes(net._handle, B, T, L_)) + (1 << 20), dtype=torch.uint8, device=dev)


def mods_ex(net, t, t_scalar, y, rows, dev, taps=True, label=False):
    """lsl_debug_mods_ex: {tfeat, hid, vec, mods[, yhid, yemb]} (taps=False: vec and mods only) and the class-6 label."""
    L, lib = _lib()
    D = net.dims.hidden
    out = {"vec": torch.full((rows, D), float("nan"), device=dev), "mods": torch.full((rows, 8 * D), float("nan"), device=dev)}
    if taps:
        out.update({"tfeat": torch.full((rows, 256), float("nan"), device=dev), "hid": torch.full((rows, D), float("nan"), device=dev)})
        if y is not None:
            out.update({"yhid": torch.full((rows, D), float("nan"), device=dev), "yemb": torch.full((rows, D), float("nan"), device=dev)})
    ws = _ws(net, rows, 1, 1, dev)

    def call():
        L.check(lib.lsl_debug_mods_ex(net._handle, _ptr(t), float(t_scalar), _ptr(y), rows, _ptr(out["vec"]), _ptr(out["mods"]), _ptr(out.get("tfeat")),
                                      _ptr(out.get("hid")), _ptr(out.get("yhid")), _ptr(out.get("yemb")), ws.data_ptr(), ws.numel(), _stream()))
    name = _labelled(net, 6, call) if label else call()
    torch.cuda.synchronize()
    return out, name


def embed(net, x, xc, mask, n, dev, stats=False, label=False):
    L, lib = _lib()
    D = net.dims.hidden
    out = {k: torch.full((n, D), float("nan"), device=dev) for k in ("cond_emb", "h", "hn")}
    if stats:
        out["stats"] = torch.full((n, 2), float("nan"), device=dev)
    ws = _ws(net, n, 1, 1, dev)

    def call():
        L.check(lib.lsl_debug_embed(net._handle, x.data_ptr(), xc.data_ptr(), mask.data_ptr(), n, 1, 1, _ptr(out["cond_emb"]), _ptr(out["h"]),
                                    _ptr(out["hn"]), _ptr(out.get("stats")), ws.data_ptr(), ws.numel(), _stream()))
    name = _labelled(net, 5, call) if label else call()
    torch.cuda.synchronize()
    return out, name


def head(net, h, mods, rows, B, tpt, dev, rec=None, x=None, noise=None, saved=None, want_trace=False, want_save=False, seed=0, offset=0, step=0,
         label=False):
    """lsl_debug_head: (out or the updated x, trace, save_out, label)."""
    L, lib = _lib()
    n, Cc = B * tpt, net.dims.in_dim
    out = torch.full((n, Cc), float("nan"), device=dev) if rec is None else x.clone()
    trace = torch.full((n, Cc), float("nan"), device=dev) if want_trace else None
    save = torch.full((n, Cc), float("nan"), device=dev) if want_save else None
    r = None
    if rec is not None:
        ax, am, aw, as_ = rec
        r = L.StepEx(0.5, ax, am, aw, as_, 0, step, -1)

    def call():
        L.check(lib.lsl_debug_head(net._handle, h.data_ptr(), mods.data_ptr(), rows, _ptr(out) if rec is not None else None,
                                   None if rec is not None else _ptr(out), C.byref(r) if r is not None else None, _ptr(noise), seed, offset,
                                   _ptr(trace), _ptr(saved), _ptr(save), B, 1, tpt, _stream()))
    name = _labelled(net, 4, call) if label else call()
    torch.cuda.synchronize()
    return out, trace, save, name


def lib_noise(net, n, seed, step, offset, dev):
    """The library's own draw of the documented stream: one no-network record x <- 0 x + 1 w of lsl_sample_ex on n trajectories of one token
    (element e of the state is element offset + e of the stream whatever the shape)."""
    L, lib = _lib()
    Cc = net.dims.in_dim
    x = torch.zeros(n, 1, 1, Cc, device=dev)
    io, keep = net.make_io(x, torch.zeros_like(x), torch.zeros(n, 1, 1, dtype=torch.long, device=dev), None)
    ws = net.workspace(n, 1, 1, dev)
    steps = (L.StepEx * 1)(L.StepEx(0.5, 0.0, 0.0, 1.0, 0.0, L.STEP_NO_NETWORK, step, -1))
    L.check(lib.lsl_sample_ex(net._handle, C.byref(io), steps, 1, None, 0, seed, offset, None, 0, ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    return x.reshape(n, Cc)


def measure(tag, got, refs, fails):
    """PARITY line of every tensor; the ones outside their bar are collected, so that a case reports all of them before it fails."""
    for k, rb in refs.items():
        assert got[k].shape == rb[0].shape or got[k].numel() == rb[0].numel(), (tag, k)
        w, i = fc.worst(got[k], rb)  # (every element: non-finite counts as infinite)
        if w < 1.0:
            parity(f"{tag}.{k}[bar]", w, 1.0)
        else:
            print(f"PARITY {tag}.{k}[bar] measured {w:.3e} bar 1.0e+00 OUTSIDE at flat index {i} of {tuple(rb[0].shape)}")
            fails.append((k, w, i, tuple(rb[0].shape)))


def guarded(fn, name):
    """A HIP error ends the run: nothing more is started on a device that has faulted."""
    t0 = time.time()
    try:
        fn()
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e) or "lamslide_hip error -10" in str(e):
            pytest.exit(f"GPU fault in {name}: {e}", returncode=3)
        raise
    print(f"FRAMECASE {name} {time.time() - t0:.2f} s")


# ---- the conditioning chain --------------------------------------------------------------------------------------------------------------
def check_mods(case, dev):
    L, lib = _lib()
    _, D, V, rows, single = case
    tag = "frame." + fc.dense_id(case)
    net, w = _net(8, D, V, False, False, dev), _weights(8, D, V, False, dev)
    t, y = fc.dense_inputs(case)
    td, yd = t.to(dev), (y.to(dev).contiguous() if y is not None else None)
    got, name = mods_ex(net, None if single else td, float(t[0]) if single else 0.0, yd, rows, dev, label=True)
    assert name == fc.mods_label(D, rows, single, V), (tag, name, fc.mods_label(D, rows, single, V))
    refs = fc.mods_references(got, t, yd, w)
    print(f"FRAMECONST {tag} tfeat {fc.ulps(got['tfeat'], refs['tfeat'][0]):.3f} hid {fc.ulps(got['hid'], refs['hid'][0]):.3f}")
    fails = []
    measure(tag, got, refs, fails)
    assert not fails, (tag, "elements outside their bar: (tensor, worst / bar, flat index, shape)", fails)
    if not single:  # lsl_debug_mods: this call without the extras, the same bits
        vec, mods = torch.empty(rows, D, device=dev), torch.empty(rows, 8 * D, device=dev)
        ws = _ws(net, rows, 1, 1, dev)
        L.check(lib.lsl_debug_mods(net._handle, td.data_ptr(), _ptr(yd), rows, vec.data_ptr(), mods.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        torch.cuda.synchronize()
        assert torch.equal(vec, got["vec"]) and torch.equal(mods, got["mods"]), tag
        bare, _ = mods_ex(net, td, 0.0, yd, rows, dev, taps=False)
        assert torch.equal(bare["vec"], got["vec"]) and torch.equal(bare["mods"], got["mods"]), tag


def check_steps(case, dev):
    L, lib = _lib()
    _, D, count = case
    tag = "frame." + fc.dense_id(case)
    net, w = _net(8, D, None, False, False, dev), _weights(8, D, None, False, dev)
    times, _ = fc.dense_inputs(case)
    mods, vec = torch.full((count, 8 * D), float("nan"), device=dev), torch.full((count, D), float("nan"), device=dev)
    ws = _ws(net, 1, 1, 1, dev)
    arr = (C.c_float * count)(*[float(v) for v in times])

    def call():
        L.check(lib.lsl_debug_mods_steps(net._handle, arr, count, mods.data_ptr(), vec.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    name = _labelled(net, 6, call)
    assert name == fc.STEPS_LABEL, (tag, name)
    singles = [mods_ex(net, None, float(times[s]), None, 1, dev, label=(s == 0)) for s in range(count)]
    assert singles[0][1] == fc.mods_label(D, 1, True), (tag, singles[0][1])
    taps = {k: torch.cat([s[0][k] for s in singles]) for k in ("tfeat", "hid", "vec", "mods")}
    # every row of the group's table: the bits of the single-row call at that time, whatever range of rows its workgroup walked
    bad = [s for s in range(count) if not (torch.equal(mods[s], taps["mods"][s]) and torch.equal(vec[s], taps["vec"][s]))]
    fails = []
    measure(tag, taps, fc.mods_references(taps, times, None, w), fails)
    assert not fails and not bad, (tag, "elements outside their bar", fails, "rows that differ from the single-row call", bad)


@pytest.mark.parametrize("case", fc.DENSE_CASES, ids=fc.dense_id)
def test_conditioning_chain_elements_against_fp64(case, dev):
    guarded(lambda: (check_mods if case[0] == "mods" else check_steps)(case, dev), fc.dense_id(case))


# ---- the embeddings ----------------------------------------------------------------------------------------------------------------------
def check_embed(case, dev):
    C_, D, n, handle = case
    tag = "frame." + fc.embed_id(case)
    normalize, lnf = handle == "norm", handle == "lnf"
    net, w = _net(C_, D, None, normalize, lnf, dev), _weights(C_, D, None, normalize, dev)
    x, xc, mask = (v.to(dev).contiguous() for v in fc.embed_inputs(case))
    got, name = embed(net, x, xc, mask, n, dev, stats=lnf, label=True)
    assert name == fc.embed_label(C_, D, n, lnf), (tag, name, fc.embed_label(C_, D, n, lnf))
    refs = {"cond_emb": fc.embed_reference(0, xc.double(), w, mask),
            "h": fc.embed_reference(1, x.double(), w, base=got["cond_emb"].double())}
    if normalize:
        refs["hn"] = fc.ln_reference(got["h"].double())
    if lnf:
        refs["stats"] = fc.stats_reference(got["h"].double())
        print(f"FRAMECONST {tag} rstd {fc.ulps(got['stats'][:, 0] / refs['stats'][0][:, 0], torch.ones(n, device=dev, dtype=torch.float64)):.3f}")
    fails = []
    measure(tag, got, refs, fails)
    del refs
    assert not fails, (tag, "elements outside their bar: (tensor, worst / bar, flat index, shape)", fails)
    assert normalize or torch.equal(got["hn"], got["h"]), (tag, "hn differs from h on a model without normalize")
    if lnf:  # the STATS instance leaves the plain instance's bits
        plain, pname = embed(_net(C_, D, None, False, False, dev), x, xc, mask, n, dev, label=True)
        assert pname == fc.embed_label(C_, D, n, False) and torch.equal(plain["h"], got["h"]) and torch.equal(plain["cond_emb"], got["cond_emb"]), tag
    if fc.embed_form(1, C_, D, n).tiles_per_wg > 1:  # a workgroup walks several tiles: ten more calls, the same bits
        for i in range(10):
            again, _ = embed(net, x, xc, mask, n, dev, stats=lnf)
            assert all(torch.equal(again[k], got[k]) for k in got), (tag, i)


@pytest.mark.parametrize("case", fc.EMBED_CASES, ids=fc.embed_id)
def test_embedding_elements_against_fp64(case, dev):
    guarded(lambda: check_embed(case, dev), fc.embed_id(case))


# ---- the output head ---------------------------------------------------------------------------------------------------------------------
def check_head(case, dev):
    D, C_, B, tpt, rows = case
    tag = "frame.head." + fc.head_id(case)
    n = B * tpt
    shared = rows == "1"
    net, w = _net(C_, D, None, False, False, dev), _weights(C_, D, None, False, dev)
    h, mods, x, noise, saved = (v.to(dev).contiguous() for v in fc.head_inputs(case))
    form = fc.head_form(D, C_, n)
    nrows = 1 if shared else B
    traj = torch.zeros(n, dtype=torch.long, device=dev) if shared else torch.arange(n, device=dev) // tpt
    shift, scale = fc.final_rows(mods, D, traj)
    mref = fc.head_reference(h.double(), shift, scale, w)
    del shift, scale
    wdev = lib_noise(net, n, fc.HEAD_SEED, fc.HEAD_STEP, fc.HEAD_OFFSET, dev)
    assert torch.isfinite(wdev).all() and float(wdev.abs().max()) > 0, tag
    got, refs, runs = {}, {}, {}
    bits = []  # bit equalities that failed: reported with the bars, behind the PARITY lines of every tensor
    for v in fc.HEAD_VARIANTS:
        rec = fc.HEAD_RECORDS.get(v)
        kw = dict(rec=rec, x=x, seed=fc.HEAD_SEED, offset=fc.HEAD_OFFSET, step=fc.HEAD_STEP)
        if v == "noise" or v == "trace":
            kw["noise"] = noise
        if v == "saved":
            kw["saved"] = saved
        if v == "trace":
            kw.update(want_trace=True, want_save=True)
        if v == "out":
            kw = {}
        out, trace, save, name = head(net, h, mods, nrows, B, tpt, dev, label=True, **kw)
        assert name == form.label, (tag, v, name, form.label)
        runs[v] = kw
        got[v] = out
        refs[v] = mref if v == "out" else fc.step_reference(mref, x.double(), rec, (wdev if v == "devnoise" else noise).double(), saved.double())
        if v == "trace" and not (torch.equal(trace, out) and torch.equal(save, out)):  # bit copies of the new state
            bits.append("trace / save_out differ from x")
    # device noise: x <- 0 x + 0 m + 1 w leaves the library's own draw, bit for bit
    pure, *_ = head(net, h, mods, nrows, B, tpt, dev, rec=(0.0, 0.0, 1.0, 0.0), x=x, seed=fc.HEAD_SEED, offset=fc.HEAD_OFFSET, step=fc.HEAD_STEP)
    if not torch.equal(pure, wdev):
        bits.append("device noise differs from the library's draw")
    other, *_ = head(net, h, mods, nrows, B, tpt, dev, rec=(0.0, 0.0, 1.0, 0.0), x=x, seed=fc.HEAD_SEED, offset=fc.HEAD_OFFSET + 1, step=fc.HEAD_STEP)
    if not torch.equal(other.reshape(-1)[:-1], wdev.reshape(-1)[1:]):
        bits.append("device noise at element offset + 1 is not the stream one element on")
    fails = []
    measure(tag, got, refs, fails)
    del refs, mref
    assert not fails and not bits, (tag, "elements outside their bar: (variant, worst / bar, flat index, shape)", fails, "bit equalities", bits)
    if shared:  # one shared row against B identical rows: the same bits
        full = mods.expand(B, -1).contiguous()
        for v in ("out", "noise"):
            out, *_ = head(net, h, full, B, B, tpt, dev, **runs[v])
            assert torch.equal(out, got[v]), (tag, v, "shared row against identical rows")
    if form.tiles_per_wg > 1:  # the prefetch and the LDS overlay across tiles: ten more calls, the same bits
        for i in range(10):
            for v in ("out", "trace"):
                out, *_ = head(net, h, mods, nrows, B, tpt, dev, **runs[v])
                assert torch.equal(out, got[v]), (tag, v, i, int((out != got[v]).any(1).sum()), "rows differ")


@pytest.mark.parametrize("case", fc.HEAD_CASES, ids=fc.head_id)
def test_head_elements_against_fp64(case, dev):
    guarded(lambda: check_head(case, dev), fc.head_id(case))


def test_hooks_refuse_what_they_cannot_run(dev):
    L, lib = _lib()
    cnet = _net(8, 192, 3, False, False, dev)  # class-conditioned
    y = torch.zeros(1, 3, device=dev)
    ws, vec, tab = _ws(cnet, 1, 1, 1, dev), torch.empty(2, 192, device=dev), torch.empty(2, 8 * 192, device=dev)
    times = (C.c_float * 2)(0.25, 0.5)
    rc = lib.lsl_debug_mods_ex(cnet._handle, None, 0.5, y.data_ptr(), 1, vec.data_ptr(), tab.data_ptr(), None, None, None, None, ws.data_ptr(),
                               ws.numel(), _stream())
    with pytest.raises(ValueError):  # the single route does not take a class vector
        L.check(rc)
    rc = lib.lsl_debug_mods_steps(cnet._handle, times, 2, tab.data_ptr(), None, ws.data_ptr(), ws.numel(), _stream())
    with pytest.raises(ValueError):  # a class-conditioned model has no groups of records
        L.check(rc)
    pnet = _net(8, 256, None, False, False, dev)
    x, xc, mask = (v.to(dev).contiguous() for v in fc.embed_inputs((8, 256, 4, "plain")))
    ws, buf, st = _ws(pnet, 4, 1, 1, dev), torch.empty(4, 256, device=dev), torch.empty(4, 2, device=dev)
    rc = lib.lsl_debug_embed(pnet._handle, x.data_ptr(), xc.data_ptr(), mask.data_ptr(), 4, 1, 1, None, buf.data_ptr(), None, st.data_ptr(),
                             ws.data_ptr(), ws.numel(), _stream())
    with pytest.raises(ValueError):  # no statistics to hand out on a plain handle
        L.check(rc)
    hnet = _net(4, 64, None, False, False, dev)
    h, mods, x, noise, saved = (v.to(dev).contiguous() for v in fc.head_inputs((64, 4, 3, 5, "B")))
    out = torch.empty(15, 4, device=dev)
    rc = lib.lsl_debug_head(hnet._handle, h.data_ptr(), mods.data_ptr(), 2, None, out.data_ptr(), None, None, 0, 0, None, None, None, 3, 1, 5, _stream())
    with pytest.raises(ValueError):  # mod_rows is 1 or B
        L.check(rc)
    rec = L.StepEx(0.5, 1.0, 1.0, 0.0, 0.5, 0, 0, -1)
    rc = lib.lsl_debug_head(hnet._handle, h.data_ptr(), mods.data_ptr(), 3, x.data_ptr(), None, C.byref(rec), None, 0, 0, None, None, None, 3, 1, 5,
                            _stream())
    with pytest.raises(ValueError):  # as without a saved state
        L.check(rc)
    torch.cuda.synchronize()
