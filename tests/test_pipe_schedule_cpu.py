"""CPU: the one decision of the batched pipeline's phase B -- which schedule the stateful tails of a step take (sindslam_amd/csrc/host/pipe_schedule.hpp,
through libsind_host.so).  The expected values are written out from the rules, not computed:
  ragged = the step has per-stream frame ranges, nact = streams with a non-empty range, few = ragged and nact <= chain_max_streams
  few and S > 1 and not depth-ahead            -> two chains
  else batch_km and not depth-ahead and not few -> rounds, split when split_rounds and S <= workers
  else                                          -> chains, over flow halves when the depth chain ran ahead
  chains run their next frame inline and poll before they sleep when S == 1 or few."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS, FLOW_CHAINS, TWO_CHAINS, ROUNDS, SPLIT_ROUNDS = range(5)

#  S  workers batch_km depth_ahead split chain_max ragged nact   schedule      inline_poll
TABLE = [
    (1,   48, False, False, True,  12, False,   1,  CHAINS,       True),     # one stream: no batched k-means
    (2,   48, True,  False, True,  12, False,   2,  SPLIT_ROUNDS, False),
    (4,    2, True,  False, True,  12, False,   4,  ROUNDS,       False),    # more streams than workers
    (128, 48, True,  False, True,  12, False, 128,  ROUNDS,       False),
    (48,  48, True,  False, True,  12, False,  48,  SPLIT_ROUNDS, False),    # S == workers still splits
    (49,  48, True,  False, True,  12, False,  49,  ROUNDS,       False),
    (2,   48, True,  False, False, 12, False,   2,  ROUNDS,       False),    # split switched off (flow_opts_off bit 16)
    (4,   48, True,  True,  True,  12, False,   4,  FLOW_CHAINS,  False),    # depth-ahead
    (128, 48, True,  True,  True,  12, False, 128,  FLOW_CHAINS,  False),
    (1,   48, False, True,  True,  12, False,   1,  FLOW_CHAINS,  True),
    (16,  48, True,  False, True,  12, True,   12,  TWO_CHAINS,   True),     # ragged, nact at chain_max_streams
    (16,  48, True,  False, True,  12, True,   13,  SPLIT_ROUNDS, False),    # ... and one above
    (128, 48, True,  False, True,  12, True,   13,  ROUNDS,       False),
    (128, 48, True,  False, True,  12, True,    1,  TWO_CHAINS,   True),
    (16,  48, True,  False, False, 12, True,   12,  TWO_CHAINS,   True),     # two chains do not depend on the split switch
    (4,   48, True,  False, True,   0, True,    3,  SPLIT_ROUNDS, False),    # chain_max_streams = 0: never chains for a step that has frames
    (4,    2, True,  False, True,   0, True,    3,  ROUNDS,       False),
    (4,   48, True,  False, True,   0, True,    0,  TWO_CHAINS,   True),     # ... a step without any frame starts nothing either way
    (4,   48, True,  True,  True,  12, True,    2,  FLOW_CHAINS,  True),     # ragged with depth-ahead: chains that run inline, with polling
    (4,   48, True,  True,  True,  12, True,    4,  FLOW_CHAINS,  True),
    (16,  48, True,  True,  True,  12, True,   13,  FLOW_CHAINS,  False),
    (1,   48, False, False, True,  12, True,    1,  CHAINS,       True),     # ragged with one stream
    (1,   48, False, False, True,   0, True,    1,  CHAINS,       True),
    (4,   48, False, False, True,  12, False,   4,  CHAINS,       False),    # several streams without batched k-means: chains that hand over
]


@pytest.fixture(scope="module")
def host():
    return C.CDLL(os.path.join(ROOT, "sindslam_amd", "libsind_host.so"))


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "S%d_w%d_km%d_da%d_sp%d_cm%d_rg%d_n%d" % tuple(int(x) for x in r[:8]))
def test_decision_table(host, row):
    poll = C.c_int(-1)
    kind = host.sindh_pipe_schedule(*[int(x) for x in row[:8]], C.byref(poll))
    assert (kind, bool(poll.value)) == (row[8], row[9]), row


def test_inline_poll_pointer_is_optional_and_names_match_the_binding(host):
    from sindslam_amd.pipeline import Pipeline, PipelineGroup
    assert host.sindh_pipe_schedule(2, 48, 1, 0, 1, 12, 0, 2, None) == SPLIT_ROUNDS
    assert Pipeline.SCHEDULES == ("chains", "flow_chains", "two_chains", "rounds", "split_rounds")
    assert callable(Pipeline.last_schedule) and callable(PipelineGroup.last_schedule)


def test_getter_without_a_gpu():
    """declared, exported, and an argument error before any device call"""
    import re
    from sindslam_amd._lib import lib
    L = lib()
    assert re.search(r"\bint sind_pipe_last_schedule\(sind_pipe\* p, int\* kind\);", open(os.path.join(ROOT, "include", "sind_hip.h")).read())
    assert L.sind_pipe_last_schedule(None, None) == -1 and b"sind_pipe_last_schedule" in L.sind_last_error()
