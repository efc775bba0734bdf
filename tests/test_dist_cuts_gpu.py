"""Partitioned collect-all rounds on cuts that are not balanced slabs (dist_cases.py; their
conditions are checked on the CPU in test_dist_case_inputs.py, their plans in
test_dist_gloo.py): every rank is a handle of its own on GPU 0, the halo moves through the
in-process transport, and every rank's estimates and flows equal the C oracle's slice for its
rows and edges by bit pattern at every stop. The stops 1 and 2 end on the flow-free rounds
(fm), 3 and 4 on the first rounds that read flows."""
import ctypes

import numpy as np
import pytest

import coracle
import fu
from dist_cases import case, plans
from err_cases import oracle_rounds
from fu.dist import DistCollectAll, run_local
from parity_util import assert_same_bits

pytestmark = pytest.mark.gpu

STOPS = (1, 2, 3, 4, 7, 20)  # rounds in total at each stop, reached by run_local calls of their own
AFTER_RESET = 5
STAGE_ROW_LIMIT = 1024  # kStageTE: kernel 8's light rows have at most min(hub_threshold, this) edges

# (case, kernel, tile_edges or None)
VARIANTS = ([(name, "recon", None) for name in ("star_hub_alone", "star_hub_alone_mega", "star_hub_first_w8",
                                                "islands_w4", "slivers_w8", "er_w8_ghost_heavy",
                                                "rmat_w8_hub_ranks")]
            + [(name, "recon", te) for name in ("slivers_w8", "star_hub_alone", "star_hub_alone_mega")
               for te in (512, 2048)]
            + [(name, "stage", None) for name in ("slivers_w8", "islands_w4", "er_w8_ghost_heavy", "star_hub_alone")]
            + [(name, "pregather", None) for name in ("rmat_w8_hub_ranks", "star_hub_alone_mega", "islands_w4")])


def no_layout(plan, kernel, options):
    """The message fu_set_option("kernel") must refuse this rank with, or None: kernel 8 needs
    a light tile (a row of at most min(hub_threshold, 1024) edges; FP::build_stage_layouts),
    kernel 9 an edge (FP::build_transpose). A partitioned handle reports it as FU_ERR_STATE."""
    if kernel == "stage":
        lim = min(options.get("hub_threshold", 128), STAGE_ROW_LIMIT)
        return None if (np.diff(plan.rowptr) <= lim).any() else r"kernel 8 \(staged slices\): no light tiles"
    if kernel == "pregather":
        return None if plan.e_local > 0 else r"kernel 9 \(pregather\): no edges"
    return None


def open_ranks(name, kernel, tile_edges):
    """Every rank's handle (kernel 4 as created), the case's options, then the kernel asked
    for: a rank without a layout for it must refuse with FU_ERR_STATE and go on with kernel 4
    (the kernels are bitwise equal, so the mixed run is compared as any other). Returns the
    handles and the kernel every rank runs."""
    c, ps = case(name), plans(name)
    engs, kernels = [], []
    for p in ps:
        e = DistCollectAll(p, c.v[p.lo:p.hi], None)
        engs.append(e)
        for key, val in c.options.items():
            fu._lib.call("fu_set_option", e._h, key.encode(), val)
        if tile_edges:
            fu._lib.call("fu_set_option", e._h, b"tile_edges", tile_edges)
        why = no_layout(p, kernel, c.options)
        if why is None:
            fu._lib.call("fu_set_option", e._h, b"kernel", fu.engine.KERNELS[kernel])
            kernels.append(kernel)
        else:
            with pytest.raises(fu.FuError, match=why) as ei:
                fu._lib.call("fu_set_option", e._h, b"kernel", fu.engine.KERNELS[kernel])
            assert ei.value.code == -4, ei.value  # FU_ERR_STATE
            kernels.append("recon")
    return engs, kernels


def check_ranks(c, ps, engs, a_ref, f_ref, what):
    for p, e in zip(ps, engs):
        assert_same_bits(e.estimates(), a_ref[p.lo:p.hi], what + ("rank", p.rank, "estimates"))
        assert_same_bits(e.flows(), f_ref[c.g.rowptr[p.lo]:c.g.rowptr[p.hi]], what + ("rank", p.rank, "flows"))


@pytest.mark.parametrize("name,kernel,tile_edges", VARIANTS)
def test_cut_cases_bitwise_at_every_stop(name, kernel, tile_edges):
    c, ps = case(name), plans(name)
    engs, kernels = open_ranks(name, kernel, tile_edges)
    try:
        assert [e.info()["kernel"] for e in engs] == kernels
        if name == "star_hub_alone" and kernel == "stage":
            assert kernels == ["stage", "stage", "recon"]  # the hub-only rank has no light tile
        if name == "islands_w4" and kernel == "pregather":
            assert kernels == ["pregather", "pregather", "recon", "pregather"]  # rank 2 has no edge
        if name == "rmat_w8_hub_ranks":
            assert kernels == [kernel] * 8 and engs[0].info()["mega_hubs"] > 0
        if name == "star_hub_alone_mega":
            assert [e.info()["mega_hubs"] for e in engs] == [0, 0, 1]
        arrays = c.g.arrays()
        done, a_ref, f_ref = 0, None, None
        for stop in STOPS:
            run_local(engs, stop - done)
            if a_ref is None:
                a_ref, f_ref = coracle.ca_sync(*arrays, c.v, stop)
            else:
                coracle.ca_rounds(*arrays, c.v, stop - done, a_ref, f_ref)
            done = stop
            check_ranks(c, ps, engs, a_ref, f_ref, (name, kernel, tile_edges, "stop", stop))
        for e in engs:  # ranks with nothing to send or to receive included
            ms = e.halo_ms()
            assert np.isfinite(ms) and ms >= 0.0, (name, kernel, ms)
        for e in engs:
            e.reset()
        run_local(engs, AFTER_RESET)
        assert [e.info()["kernel"] for e in engs] == kernels
        a_ref, f_ref = coracle.ca_sync(*arrays, c.v, AFTER_RESET)
        check_ranks(c, ps, engs, a_ref, f_ref, (name, kernel, tile_edges, "after reset"))
    finally:
        for e in engs:
            e.close()


@pytest.mark.parametrize("shift", [0.0, 1.0])
def test_islands_error_trace_per_rank(shift):
    """islands_w4 with the check on every round, four rounds, each followed by the exchange:
    every rank's entry is the maximum of |a - target| over its own rows, and the maximum over
    the ranks is the oracle's, by bit pattern. The targets are the component means of the
    global graph, plus `shift`. With shift 0 the rank without edges reports +0.0: a row of
    degree 0 keeps its value as its estimate, and its component mean is that value. With
    shift 1 its entry is its own rows' |v - (v + 1)|: neither 0 nor NaN, and not the global
    maximum."""
    c, ps = case("islands_w4"), plans("islands_w4")
    mean, _ = fu.component_means(c.g.rowptr, c.g.col, c.v)
    target = mean + shift
    R = 4
    a_rounds = oracle_rounds(c.g.arrays(), c.v, R, nthreads=1)
    engs = [DistCollectAll(p, c.v[p.lo:p.hi], None) for p in ps]
    try:
        arr = (ctypes.c_void_p * c.world)(*[e._h.value for e in engs])
        for p, e in zip(ps, engs):
            e.set_targets(target[p.lo:p.hi])
        got = np.empty((R, c.world))
        for r in range(R):
            for q, e in enumerate(engs):
                got[r, q] = e.run(1, err_every=1)[0]
            fu._lib.call("fu_dist_exchange_local", arr, c.world)
        want = np.stack([np.abs(a_rounds[:, p.lo:p.hi] - target[p.lo:p.hi]).max(axis=1) for p in ps], axis=1)
        for p in ps:
            assert_same_bits(np.ascontiguousarray(got[:, p.rank]), np.ascontiguousarray(want[:, p.rank]),
                             ("rank", p.rank, "shift", shift))
        assert_same_bits(got.max(axis=1), np.abs(a_rounds - target).max(axis=1), ("all ranks", shift))
        lone = got[:, 2]  # the rank without edges
        assert not np.isnan(lone).any()
        if shift:
            assert (lone > 0).all() and (lone < got.max(axis=1)).all()
        else:
            assert (lone == 0).all() and not np.signbit(lone).any()
        for p, e in zip(ps, engs):
            assert_same_bits(e.estimates(), a_rounds[-1, p.lo:p.hi], ("rank", p.rank))
    finally:
        for e in engs:
            e.close()
