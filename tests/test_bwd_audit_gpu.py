"""The stage audit of the generic training backward on the GPU: one native.decoder_forward_train into a tape,
then for every site of the backward's launch list one native.decoder_backward(until=site) into a scratch and gradient destinations
pre-filled with 0xFF / NaN, and what that site wrote compared element by element with the fp64 evaluation of the operands it read
(tests/bwd_audit_util.py: references, bars and their derivation; the host file shows that the references are autograd through the
oracle, that the bars can be met and that they catch each kind of fault).  The cases and option sets are section 29's: every option
set that the library accepts, the head dims of every tile count, dropout, and ragged batches with NaN in all padding.
Run on the GPU box: python -m pytest tests -m gpu."""
import pytest
import torch

import bwd_audit_util as BA
import dropout_util as DU
import tape_audit_util as TA
import tape_bf16_util as TU
import test_tape_audit_gpu as FWD
import train_bf16_util as U
import train_ragged_util as R
from edge_diffusion_tts_amd import native

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = FWD.IDS
opt_sets = FWD.opt_sets
cu = FWD.cu


class Run:
    """A training forward into a tape, and truncated backwards from it."""

    def __init__(self, cs, opts, drop=None, nan_padding=True, **kw):
        self.cs, self.drop = cs, drop
        self.dec = dec = FWD.make(cs, opts, dropout=None if drop is None else drop[0], **kw)
        self.dims, self.packed = dec.dims(), dec._ensure_packed()
        cfg, B, T, S = cs.cfg, cs.B, cs.T, cs.S
        self.inp = inp = FWD.padded(cs)
        self.ws = dec.workspace(B, T, S, B, DEV)
        self.tape = torch.full((native.train_tape_bytes(self.dims, B, T, S),), 0xFF, dtype=torch.uint8, device=DEV)
        self.sem = None if inp["f"] is not None else cu(inp["sem"])
        self.x, self.t, self.si, self.f = cu(inp["x"]), cu(inp["t"]), cu(inp["si"]), cu(inp["f"])
        self.lens = (cu(cs.t_len), cu(cs.s_len))
        native.decoder_forward_train(self.dims, self.packed, self.ws, self.tape, self.x, self.t, self.si, self.sem, self.f, S, drop, *self.lens)
        d_eps = BA.d_eps_of(cs)
        if cs.t_len is not None and nan_padding:
            d_eps = d_eps.masked_fill(~R.frame_mask(cs.t_len, T), float("nan"))
        self.d_eps_cpu, self.d_eps = d_eps, cu(d_eps)
        # gradient destinations as EdgeDiffusionDecoder's backward hands them over: what torch would leave without a gradient gets none
        params = dict(dec.named_parameters())
        self.grads = {n: torch.empty_like(p) for n, p in params.items() if dec._enters_output(n, inp["f"] is not None, inp["si"] is not None)}
        self.slots = [self.grads.get(dec._slot_param(n)) for n in native.slot_names(cfg.layers)]
        self.d_x = torch.empty_like(self.x)
        self.d_sem = None if self.f is None else torch.empty_like(self.f)
        self.scratch = torch.empty(native.train_scratch_bytes(self.dims, B, T, S), dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        assert native.index_errors(self.ws) == 0

    def tape_dict(self):
        cs, opts_tape = self.cs, self.dec.tape_dtype == "bf16"

        def region(layer, which):
            r = TU.tape_region(self.tape, self.dims, cs.cfg, cs.B, cs.T, cs.S, layer, which)
            assert r.dtype == (torch.bfloat16 if opts_tape and which in TU.NARROWED else torch.float32), which
            return r.to(torch.float64).cpu()

        tp = {w: region(0, w) for w in native.TAPE_GLOBALS}
        tp["layers"] = [{w: region(l, w) for w in native.TAPE_REGIONS} for l in range(cs.cfg.layers)]
        return tp

    def destinations(self):
        return list(self.grads.values()) + [self.d_x] + ([] if self.d_sem is None else [self.d_sem])

    def fill(self, value=float("nan")):
        self.scratch.fill_(0xFF)
        for g in self.destinations():
            g.fill_(value)

    def backward(self, until=None):
        native.decoder_backward(self.dims, self.packed, self.ws, self.tape, self.x, self.t, self.si, self.sem, self.f, self.cs.S, self.d_eps,
                                self.slots, self.d_x, self.d_sem, self.drop, *self.lens, scratch=self.scratch, until=until)

    def region(self, name, shape):
        off, n = native.train_scratch_region(self.dims, self.cs.B, self.cs.T, self.cs.S, name)
        flat = self.scratch[off:off + n].view(torch.float32)
        assert shape[0] * shape[1] <= flat.numel(), (name, shape, flat.numel())
        return flat[:shape[0] * shape[1]].reshape(shape)  # (`big` is used at two pitches; every other member is filled whole)

    def read(self, name, shape):
        if name == "d_x":
            v = self.d_x.reshape(shape)
        elif name == "d_sem":
            v = self.d_sem.reshape(shape)
        elif name.startswith("g:"):
            v = self.grads[name[2:]]
            assert tuple(v.shape) == tuple(shape), (name, v.shape, shape)
        else:
            v = self.region(name, shape)
        return v.to(torch.float64).cpu()

    def producer(self):
        def produce(key, st, shapes):
            self.fill()
            self.backward(until=key)
            return {nm: self.read(nm, shape) for nm, shape in shapes.items()}
        return produce


def audit(cs, opts, what, drop=None, **kw):
    run = Run(cs, opts, drop, **kw)
    mult = None
    if drop is not None:
        p, seed = drop
        mult = {(l, site): native.dropout_mask(run.dims, site, l, cs.B, cs.T, cs.S, p, seed, DEV).to(torch.float64).cpu() * DU.scale(p)
                for l in range(cs.cfg.layers) for site in range(4)}
        assert all(0 < int((m != 0).sum()) < m.numel() for m in mult.values())
    cx = BA.Ctx(cs._replace(inp=run.inp), opts, run.tape_dict(), mult, d_eps=run.d_eps_cpu)
    res = BA.audit(cx, run.producer())
    assert native.index_errors(run.ws) == 0
    by = BA.check(res, what)
    return run, cx, by


# ------------------------------------------------------------------------------------------------------------ 1. every site, every option set
@opt_sets
@pytest.mark.parametrize("name", TA.PLAIN)
def test_every_site_is_within_its_bar(name, opts):
    cs = TA.case(name)
    _, cx, by = audit(cs, opts, f"{name} {IDS[opts]}")
    assert set(by) == {s for _, s in cx.sites()}


@opt_sets
@pytest.mark.parametrize("name", TA.DROPPED)
def test_every_site_is_within_its_bar_under_dropout(name, opts):
    """The multipliers are the library's own masks (native.dropout_mask, which tests/test_dropout_gpu.py shows equal to dropout_util's)
    times dropout_util's scale."""
    cs = TA.case(name)
    _, cx, by = audit(cs, opts, f"{name} p={U.DROP_P} {IDS[opts]}", drop=(U.DROP_P, U.drop_seeds()[0]))
    assert "dropdown" in by


@opt_sets
@pytest.mark.parametrize("name", TA.RAGGED)
def test_every_live_element_of_a_ragged_batch_is_within_its_bar(name, opts):
    """NaN in all padding of x, sem_features and d_eps, 0xFF in the tape and the scratch: only live rows are compared (and must have
    been written), the references read rows < T_b and < S_b only, the dead rows of every dX that the launch list zeroes are exactly
    0, and so are d_x and d_sem_features past the lengths."""
    cs = TA.case(name)
    run, cx, _ = audit(cs, opts, f"{name} {IDS[opts]}", train_lengths=True)
    run.fill()
    run.backward()
    torch.cuda.synchronize()
    for g, lens, n in ((run.d_x, cs.t_len, cs.T), (run.d_sem, cs.s_len, cs.S)):
        dead = ~R.frame_mask(lens, n).expand_as(g)
        assert bool(torch.isfinite(g).all()) and not bool(g.cpu()[dead].any()) and int(dead.sum()) > 0
    assert all(bool(torch.isfinite(g).all()) for g in run.destinations())


# ------------------------------------------------------------------------------------------------------------ 2. until the last site == the whole call
@opt_sets
@pytest.mark.parametrize("name", ("G4", "R4"))
def test_until_the_last_site_is_the_whole_backward(name, opts):
    cs = TA.case(name)
    run = Run(cs, opts, train_lengths=cs.t_len is not None)
    last = BA.Ctx(cs, opts, run.tape_dict()).sites()[-1]
    assert last == (0, "time")
    run.fill()
    run.backward()
    whole = [g.clone() for g in run.destinations()]
    run.fill()
    run.backward(until=last)
    torch.cuda.synchronize()
    assert len(whole) == len(run.grads) + 2
    for a, b in zip(whole, run.destinations()):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    # ... by number as well as by name
    run.fill()
    run.backward(until=(0, native.BWD_SITES.index("time")))
    for a, b in zip(whole, run.destinations()):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 3. later sites are not run
def test_a_stopped_call_leaves_later_destinations_untouched():
    cs, opts = TA.case("G2"), TA.OPTION_SETS[0]
    run = Run(cs, opts)
    cx = BA.Ctx(cs, opts, run.tape_dict())
    sites = cx.sites()
    stop = sites.index((cs.cfg.layers - 1, "n3"))
    # what the sites up to the stop write, from the references' own list of outputs
    st, written = {}, set()
    ref = BA.Ref(cx)
    for key in sites[:stop + 1]:
        outs = BA._site(cx, key, st, ref)
        written |= set(outs)
        st.update({nm: o.ref for nm, o in outs.items()})
    SENTINEL = 12345.0
    run.fill(SENTINEL)
    run.backward(until=sites[stop])
    torch.cuda.synchronize()
    names = {("g:" + n): g for n, g in run.grads.items()}
    names.update(d_x=run.d_x, d_sem=run.d_sem)
    assert {n for n in names if n in written} == {n for n in written if n.startswith("g:")} and len(written) > 8
    for n, g in names.items():
        if n in written:
            assert not bool((g == SENTINEL).any()) and bool(torch.isfinite(g).all()), n
        else:
            assert bool((g == SENTINEL).all()), n
    # ... and the scratch members that only later sites write still hold 0xFF (stat and part are working space of many sites)
    for member in set(native.SCRATCH_REGIONS) - written - {"stat", "part"}:
        off, n = native.train_scratch_region(run.dims, cs.B, cs.T, cs.S, member)
        assert bool((run.scratch[off:off + n] == 0xFF).all()), member
    assert {"dtc", "e", "a1", "u1", "du1", "dkv", "crn", "dcr", "dcp"} <= set(native.SCRATCH_REGIONS) - written


# ------------------------------------------------------------------------------------------------------------ 4. errors
def test_a_bad_layer_or_site_is_an_argument_error():
    cs, opts = TA.case("G2"), TA.OPTION_SETS[0]
    run = Run(cs, opts)
    L = cs.cfg.layers
    run.fill(7.0)
    bad = [(L, "down"), (-1, "down"), (0, len(native.BWD_SITES)), (0, -1), (1, "out"), (1, "time"),
           (0, "dropdown")]  # (no dropout in this call)
    for until in bad:
        with pytest.raises(native.EdttsError, match="edtts_decoder_backward_until"):
            run.backward(until=until)
    plain = TA.case("G1")  # plain RMSNorm blocks: no AdaLN projections and no time-path gradient
    r1 = Run(plain, opts)
    for site in ("ada", "step", "time"):
        with pytest.raises(native.EdttsError, match="edtts_decoder_backward_until"):
            r1.backward(until=(0, site))
    nostep = TA.case("G3")  # no step_idx: no step_emb scatter
    r3 = Run(nostep, opts)
    with pytest.raises(native.EdttsError, match="edtts_decoder_backward_until"):
        r3.backward(until=(0, "step"))
    torch.cuda.synchronize()
    assert all(bool((g == 7.0).all()) for g in run.destinations())  # a refused call launches nothing
