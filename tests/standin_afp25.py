"""The stand-in engine of tests/standin_openings.py with the one name afp25.label_bases calls besides: gt_inverse, the oracle's inversion
row by row.  hash_to_g1 (tests/standin_member.py, from the Python oracle) and multi_pair_fixed_q (tests/standin_engine.py, a plain
multi-pairing over the repeated list) are inherited.  Nothing here shares code with the kernels or with the planners' sequence of calls."""
import numpy as np

from standin_openings import OpeningsStandIn


class SchemeStandIn(OpeningsStandIn):
    def gt_inverse(self, a):
        return np.asarray(self.o.gt_inverse(np.asarray(a, dtype=np.uint8).reshape(-1))).reshape(-1, 384)


class Untouchable:
    """an engine no planner may reach: a ValueError that is due before the first engine call is raised without it"""

    def __getattr__(self, name):
        raise AssertionError("the engine was touched (%s) before the arguments were refused" % name)
