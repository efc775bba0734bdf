"""The round skeleton that fu.CollectAllLossy and fu.CollectAllChurn share (csrc/fu_rev_round.h),
through both of its rules at once: with no loss and no mask every lossy slot gathers from round 1
on, and with everything alive every churn slot does, so the two engines and coracle.ca_sync hold
the same bits in estimates and flows after every one of rounds 0 to 5 (round 0 is the lossy
engine's zero round and the churn engine's all-FRESH round).

The graphs are the smallest on which both engines take the shared light path, the shared heavy
path and the chunk carry: lossy_cases.tile_limit_graph() closes its light tiles in every way, and
churn_cases.chunk_edge_graph() has a row one slot above the heavy threshold (129) and a row of
one chunk and one slot (2049). Neither is a star."""
import numpy as np
import pytest

import coracle
import fu
from churn_cases import HEAVY_CHUNK, chunk_edge_graph, tile_limit_graph
from lossy_cases import TILE_HEAVY_DEG
from parity_util import assert_same_bits

pytestmark = pytest.mark.gpu

ROUNDS = 6


@pytest.mark.parametrize("graph", [tile_limit_graph, chunk_edge_graph], ids=["tile_limit", "chunk_edge"])
def test_lossless_lossy_and_all_alive_churn_are_one_round(graph):
    g = graph()
    if graph is chunk_edge_graph:
        assert {TILE_HEAVY_DEG + 1, HEAVY_CHUNK + 1} <= {int(d) for d in g.degrees}
    v = fu.uniform_values(g.n, seed=6)
    a_ref, f_ref = coracle.ca_sync(*g.arrays(), v, 1)
    with fu.CollectAllLossy(g, v, loss=0.0) as lossy, fu.CollectAllChurn(g, v) as churn:
        for r in range(ROUNDS):
            lossy.run(1)
            churn.run(1)
            for name, eng in (("lossy", lossy), ("churn", churn)):
                assert_same_bits(eng.estimates(), a_ref, (name, "estimates after round", r))
                assert_same_bits(eng.flows(), f_ref, (name, "flows after round", r))
            assert_same_bits(churn.estimates(), lossy.estimates(), ("churn against lossy, estimates", r))
            assert_same_bits(churn.flows(), lossy.flows(), ("churn against lossy, flows", r))
            coracle.ca_rounds(*g.arrays(), v, 1, a_ref, f_ref)
        assert lossy.stats[1] == 0  # no message lost
