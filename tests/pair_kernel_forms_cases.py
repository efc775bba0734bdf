"""Shared by test_pair_kernel_forms_gpu.py and test_pair_kernel_forms_case_inputs.py: two shapes of
the pair engine's kernels (csrc/fu_pair.hip) that the widths of pair_columns_cases leave out.

1. kp_exchange_cols gives lane l of a pair's group the columns l and l + 8. At the widths of
   LIGHT_WIDTHS the lanes that carry a column all carry one or all carry two; at K = 9 lane 0
   alone has a second column and at K = 15 lane 7 alone has none.
2. kp_heavy<Args, false>, the heavy kernel of a K-column handle, at K = 1 (HEAVY_WIDTHS starts at
   2, and a scalar handle runs kp_heavy<Args, true>) and at K = 9 and 15 again: on
   pair_columns_cases.boundary_graph, whose centres sit on the chunk edges of that K.

Everything is built from pair_columns_cases' helpers; the conditions that make the inputs
meaningful are asserted in test_pair_kernel_forms_case_inputs.py. Nothing here runs the engine.
"""
from pair_columns_cases import boundary_graph

MIXED_WIDTHS = (9, 15)              # 1.: a group's lanes disagree on having a second column
HEAVY_FORM_WIDTHS = (1, 9, 15)      # 2.

# The runs of 2. on heavy_graph(K): BOUNDARY_ROUNDS rounds at the matching seed HEAVY_SEED[K],
# within which every centre both initiates and listens; at CLASS_P and the loss seed
# HEAVY_LOSS_SEED[K] each of the three outcomes occurs on a pair whose initiator's row is heavy
# and on one whose listener's row is. Found by a search over seeds on the host.
HEAVY_SEED = {1: 1, 9: 1, 15: 1}
HEAVY_LOSS_SEED = {1: 5, 9: 5, 15: 5}

# boundary_graph draws a centre's leaves without repeats: the widest centre has 2 * 2048 / K + 1.
HEAVY_LEAVES = {1: 5000, 9: 3000, 15: 3000}


def heavy_graph(K):
    return boundary_graph(K, HEAVY_LEAVES[K])
