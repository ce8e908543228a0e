"""The smallest fp32 shapes that reach every merge and select instantiation of csrc/topk_merge.h through hcir_sim_topk.

Shared by tests/test_sim_plan_host.py (CPU: the routes of each shape, derived from csrc/sim_plan.h, must be exactly the
set written here, and the union must be every instantiation in the build) and tests/test_sim_topk_gpu.py (GPU: each
shape bit-exact against the C oracle).  A route is (kernel, lists or slots per lane): the kernel's template argument.
The gated fallback launches of the candidate flow count: they are launched (and exit at once) on every call."""

# every merge / select instantiation csrc/sim_topk.hip can launch from hcir_sim_topk
INSTANTIATIONS = {("merge32q", 1), ("merge32q", 2), ("merge32q", 3), ("merge32q", 4), ("merge32", 9), ("merge_sel", 9),
                  ("select", 8), ("select", 16), ("select4", 13)}

# ((nq, ng, d, k), routes reached, what the shape is there for)
ROUTE_SHAPES = [
    ((5, 1000, 8, 10), {("merge32q", 1)}, "single scan, 4 lists"),
    ((40, 60000, 8, 10), {("merge32q", 1), ("merge32q", 2)},
     "two phases on 128-row tiles: 64 prefix lists, then 405 + the prefix list"),
    ((40, 90000, 8, 10), {("merge32q", 1), ("merge32q", 3)}, "640 + the prefix list"),
    ((40, 120000, 8, 10), {("merge32q", 1), ("merge32q", 4)},
     "768 + the prefix list, which is list 768: the LAST slot (j = 3) of lane 0 of wave 0"),
    ((5, 1000, 8, 20), {("merge32", 9)}, "single scan, kout > 16"),
    ((3, 2000, 8, 100), {("merge32", 9)}, "two passes of 64 and 36 ranks: kth_idx and the pass copy"),
    ((3, 2000, 8, 70), {("merge32", 9), ("merge32q", 1)}, "a last pass of 6 ranks takes the four-wave merge"),
    ((8, 40000, 8, 20), {("merge_sel", 9), ("select4", 13), ("merge32", 9)}, "candidate flow, 2 groups, 3008 slots"),
    ((4, 40000, 8, 10), {("merge32q", 1), ("select", 8)}, "candidate flow, one floor, 448 slots"),
    ((4, 1600000, 8, 10), {("merge32q", 2), ("select", 16), ("merge32q", 3)},
     "the prefix is capped at 131072 rows, so 960 slots; a 51 MB gallery"),
    ((2, 20, 8, 20), {("merge32", 9)}, "k = ng: lists shorter than k, the -inf / -1 entries of the reader and writer"),
]
