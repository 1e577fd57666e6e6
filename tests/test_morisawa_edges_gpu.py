"""The Morisawa families on the device at the edge fleet of tests/morisawa_edges.py: B = 67 gaits with a model, a height and times of
their own whose largest argument omega_j dT_j runs from 8 to the admission bound WG_MORISAWA_WALK_ARG_MAX -- from 10.75 on mo_exp
multiplies by 2^16 (k >= 16), which no other device test reaches --, lies on the bound from both sides and beyond it (refused:
ordinary status returns, nothing here is expected to fault).  smax = 3 (short) and 15 (long, the smallest size only that family takes).

Against the host twins by bytes with canary rows around every array (the Dev class of tests/test_morisawa_gpu.py), the re-plan
against host twin and full solve by bytes, and the device's own samples against the 50-digit restatement tests/morisawa.py under the
rule of tests/test_morisawa_host.py: within 16 x d_ref, and 16 x d_ref < 1e-8 m.

Measured on an MI355X (figures also in DESIGN.md 3.13), the four admitted gaits nearest the bound:
  short (S = 3, 3, 3, 2; arguments 13.5, 13.5, 13.34, 13.25): d_ref = 1.5e-10 m, device 3.6e-11 m, bound 2.4e-9 m
  long (S = 10, 13, 12, 4; the same arguments): d_ref = 1.4e-10 m, device 2.1e-10 m, bound 2.3e-9 m
The six tests take 3.7 s."""
import functools

import numpy as np
import pytest

import morisawa as mo
import morisawa_edges as me
import morisawa_fleets as mf
import morisawa_replan as rp
from test_morisawa_gpu import SENT_D, Dev, to_dev
from test_morisawa_host import D_REF_CEILING, D_REF_FACTOR

wg = mf.wg()
pytestmark = pytest.mark.gpu

FAMILIES = pytest.mark.parametrize("long_,smax", ((False, 3), (True, 15)), ids=("short", "long"))


@functools.lru_cache(maxsize=None)
def case(long_, smax):
    """the edge fleet and what the host twins make of it with its per-gait models; never modified"""
    fam = rp.Family(long_)
    f = me.edge_fleet(smax)
    t0 = 0.2                                                    # inside every gait's first interval (the shortest is 0.3 s)
    refused = tuple(b for b in range(f.B) if not f.admitted[b])
    blocks, status = fam.solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, smax, blocks=np.full((f.B, fam.words(smax)), SENT_D))
    assert tuple(b for b in range(f.B) if status[b] != 0) == refused and all(status[b] == wg.MORISAWA_BAD_INPUT for b in refused)
    lcap = max(fam.length(f.models[b], int(f.n_steps[b]), t0) for b in range(f.B) if f.admitted[b]) + 3
    samples = fam.sample(blocks, status, smax, t0, f.model.T, lcap)
    lens = samples["length"]
    assert all(lens[b] == wg.MORISAWA_BAD_INPUT for b in refused) and all(lens[b] > 100 for b in range(f.B) if f.admitted[b])
    return dict(fam=fam, fleet=f, t0=t0, refused=refused, blocks=blocks, status=status, lcap=lcap, samples=samples, words=fam.words(smax))


@FAMILIES
def test_edge_fleet_gives_the_host_twins_bytes(long_, smax):
    """_solve_dev with the per-gait models, then _sample_dev, then _walk_dev: blocks, statuses, lengths and every output are the host
    twin's bytes; the refused gaits' blocks and columns are still the canaries"""
    c = case(long_, smax)
    fam, f = c["fam"], c["fleet"]
    d = Dev(f, c["words"], c["lcap"])
    fam.solve_dev(*d.solve_args())
    d.check_blocks(c["blocks"], c["status"], refused=c["refused"])
    fam.sample_dev(f.B, smax, d.blocks[1:].data_ptr(), d.status[1:].data_ptr(), c["t0"], f.model.T, c["lcap"], d.out_ptrs(), d.length[1:].data_ptr())
    d.check_outs(c["samples"], refused=c["refused"])
    w = Dev(f, c["words"], c["lcap"])
    fam.walk_dev(w.models.data_ptr(), f.B, smax, *w.solve_args()[3:], c["t0"], c["lcap"], w.out_ptrs(), w.length[1:].data_ptr(), T=f.model.T)
    w.check_blocks(c["blocks"], c["status"], refused=c["refused"])
    w.check_outs(c["samples"], refused=c["refused"])


@FAMILIES
def test_edge_replan(long_, smax):
    """five plans on the timing of an edge gait -- the admitted one nearest the bound -- re-planned on the device from that gait's
    block, which the device's own fleet solve made: device re-plan == host twin == the device's full solve, by bytes"""
    import torch
    c = case(long_, smax)
    fam, e = c["fam"], c["fleet"]
    src = me.nearest_admitted(e, 1)[0]
    S = int(e.n_steps[src])
    f = rp.plans(5, smax, S, 2100 + smax, height=float(e.com0[src, 2]))
    for m in [f.model] + [f.models[b] for b in range(5)]:
        m.t_single, m.t_double = e.models[src].t_single, e.models[src].t_double
    for i in range(smax):                                       # plan 0 is the edge gait's own
        f.steps[i] = e.steps[src * smax + i]
    f.triples[0], f.init_feet[0], f.com0[0, :2] = e.triples[src], e.init_feet[src], e.com0[src, :2]
    assert me.argument(f.com0[0, 2], f.model.t_single, f.model.t_double) == e.arg[src] >= e.bound * (1 - 1e-12)
    full_host, st = fam.solve(f.model, f.steps, f.n_steps, f.init_feet, f.com0, smax)
    assert list(st) == [0] * 5
    twin, st = fam.resolve(f.model, full_host[0:1], None, f.steps, f.init_feet, f.com0, smax)
    assert list(st) == [0] * 5 and twin.tobytes() == full_host.tobytes()
    fac = Dev(e, c["words"], 1)                                 # the edge fleet's blocks on the device: gait src is the factor block
    fam.solve_dev(*fac.solve_args())
    full, d = Dev(f, c["words"], 1), Dev(f, c["words"], 1)
    fam.solve_dev(*full.solve_args(f.model))
    fo = to_dev(np.full(5, src, np.int32))
    fam.resolve_dev(f.model, 5, smax, fac.blocks[1:].data_ptr(), e.B, fo.data_ptr(), d.steps.data_ptr(), d.feet.data_ptr(),
                    d.com0.data_ptr(), d.blocks[1:].data_ptr(), d.status[1:].data_ptr())
    d.check_blocks(twin, [0] * 5)
    full.check_blocks(twin, [0] * 5)
    assert torch.equal(d.blocks.view(torch.int64), full.blocks.view(torch.int64))
    # a refused edge gait's block is no factor: it still holds the canaries
    bad = to_dev(np.full(5, c["refused"][0], np.int32))
    r = Dev(f, c["words"], 1)
    fam.resolve_dev(f.model, 5, smax, fac.blocks[1:].data_ptr(), e.B, bad.data_ptr(), r.steps.data_ptr(), r.feet.data_ptr(),
                    r.com0.data_ptr(), r.blocks[1:].data_ptr(), r.status[1:].data_ptr())
    r.check_blocks(twin, [wg.MORISAWA_BAD_INPUT] * 5, refused=range(5))


@FAMILIES
def test_device_samples_against_the_truth(long_, smax):
    """the four admitted gaits nearest the bound: the device's own samples (walk_dev, a model per gait) against the 50-digit
    restatement at every sample where the interval changes, the last and about 40 others; d_ref over the four gaits"""
    import torch
    c = case(long_, smax)
    fam, f = c["fam"], c["fleet"]
    d = Dev(f, c["words"], c["lcap"])
    fam.walk_dev(d.models.data_ptr(), f.B, smax, *d.solve_args()[3:], c["t0"], c["lcap"], d.out_ptrs(), d.length[1:].data_ptr(), T=f.model.T)
    torch.cuda.synchronize()
    lens = d.length.cpu().numpy()[1:-1]
    r = {k: v.cpu().numpy()[1:-1] for k, v in d.outs.items()}
    d_ref = d_dev = 0.0
    for b in me.nearest_admitted(f, 4):
        assert f.arg[b] > f.bound - 0.5 and lens[b] == c["samples"]["length"][b]
        ks, tv, v64, nat = me.truth_samples(mo, f, b, c["t0"], int(lens[b]), between=40)
        got = me.sampled_columns(r, ks, b)
        assert [(r["left_type"][k, b], r["right_type"][k, b]) for k in ks] == nat
        d_ref, d_dev = max(d_ref, float(np.abs(v64 - tv).max())), max(d_dev, float(np.abs(got - tv).max()))
        print("gait %d (%s, S = %d, argument %.12g): d_ref %.3g, device %.3g" %
              (b, f.route[b], f.n_steps[b], f.arg[b], float(np.abs(v64 - tv).max()), float(np.abs(got - tv).max())))
    print("%s d_ref %.3g, device %.3g, bound %.3g" % (fam.name, d_ref, d_dev, D_REF_FACTOR * d_ref))
    assert D_REF_FACTOR * d_ref < D_REF_CEILING
    assert d_dev <= D_REF_FACTOR * d_ref
