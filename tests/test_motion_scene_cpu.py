"""CPU: what test_pipeline_motion_gpu.py and the sequence test rely on, from the ORACLE alone -- the flag table of the scene streams, and the conditions under
which a pipeline that scatters the second DeepFlow pass to a wrong slot, or refines against the wrong frame, cannot pass: mixed steps, flagged[k] != k, an
all-flagged next to an unflagged slice, a flag that changes inside a step, and flagged frames whose imgDyna changes with the flow path."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import motion_scene as M
import oracle_lib as O


def _measured():
    keys = sorted({(c[0], c[1], s) for c in M.CONFIGS.values() for s in c[5]} | set(M.FLAGS), key=repr)
    O.lib()
    with ThreadPoolExecutor(8) as ex:
        got = list(ex.map(lambda k: M.oracle_flags(k[0], k[1], k[2], 1 + len(M.FLAGS[k])), keys))
    return dict(zip(keys, got))


def test_flag_table_and_the_conditions_of_the_pipeline_test():
    meas = _measured()
    for k, v in meas.items():
        print("flags", k, " ".join(str(x) for x in v))
        assert v == M.FLAGS[k], (k, v, M.FLAGS[k])
    flags = {n: M.config_flags(n, lambda w, h, what: meas[(w, h, what)]) for n in M.CONFIGS}
    # (a) every tested step of a batch holds a flagged and an unflagged pair (the one-pair handle takes both values over its two steps)
    for n, steps in flags.items():
        if M.CONFIGS[n][2] * M.CONFIGS[n][3] > 1:
            assert all(set(st) == {0, 1} for st in steps), (n, steps)
    assert flags["one_one"] == [[1], [0]]
    assert flags["one_slice"] == [[0, 0, 1, 1, 0, 0, 1, 1]] * 2
    # (b) pair 0 unflagged and a later pair flagged: flagged[k] != k
    assert any(st[0] == 0 and 1 in st for n in ("one_slice", "slices_clean", "slices_mixed") for st in flags[n])
    # (c) one slice without a flagged pair next to one that holds only flagged pairs; and a configuration whose two slices are both mixed
    for st in flags["slices_clean"]:
        assert st[:4] == [0, 0, 0, 0] and st[4:] == [1, 1, 1, 1]
    assert all(set(st[:4]) == {0, 1} and set(st[4:]) == {0, 1} for st in flags["slices_mixed"])
    # three slices of two pairs: the last one holds fewer flagged pairs than pairs, another one none, another one only flagged pairs
    assert flags["three_slices"][0] == [1, 1, 0, 0, 1, 0]
    # (d) a stream changes its flag between t and t + 1 of one step
    T = 2
    assert any(st[k] != st[k + 1] for n in ("slices_mixed", "three_slices", "walkers") for st in flags[n] for k in range(0, len(st), T))
    # ragged step (2, 1, 0, 2 active frames of the second step): the frames that run hold both flags
    st = flags[M.RAGGED][1]; ran = [st[0], st[1], st[2], st[6], st[7]]
    assert set(ran) == {0, 1}


def test_flagged_frames_depend_on_the_flow_path():
    """(e) flagged frames on which the oracle's imgDyna holds both 255 and 0, and on which it changes when the first path's flow (flow(n, n-2) refined against
    frame n-2: what a pair keeps if the second pass lands in another slot or is never chosen) is fed instead; on unflagged frames the two flows are the same bits"""
    cases = [(192, 144, (6, 2, "block"), 3), (192, 144, (8, 0, "block"), 2), (192, 144, (8, 0, "block"), 3), (320, 240, ("walkers", 0), 2), (320, 240, ("walkers", 1), 3),
             (192, 144, (0, 0), 2)]
    O.lib()
    with ThreadPoolExecutor(6) as ex:
        flows = list(ex.map(lambda c: M.path_flows(*c), cases))
    changed = {}
    for (w, h, what, f), (full, first, flag) in zip(cases, flows):
        assert flag == M.FLAGS[(w, h, what)][f - 2]
        if not flag:
            assert np.array_equal(full, first), (what, f)
            continue
        assert not np.array_equal(full, first) or what == (0, 0), (what, f)
        b, d = M.stream(w, h, what); K = M.intrinsics(w)
        good = O.DynaDetect(b[f - 1], b[f - 2], *K).detect_with_flow(b[f], d[f], full)
        bad = O.DynaDetect(b[f - 1], b[f - 2], *K).detect_with_flow(b[f], d[f], first)
        if what != (0, 0):
            assert (good[0] == 255).any() and (good[0] == 0).any(), (what, f)
        changed[(w, what, f)] = int((good[0] != bad[0]).sum())
    print("imgDyna pixels that change with the flow path:", changed)
    assert all(v > 0 for k, v in changed.items() if k[1] != (0, 0)), changed
    assert changed[(192, (0, 0), 2)] == 0                   # the static pan stream pins the flag only: zero flow along either path


def test_sequence_flags_change_inside_a_chunk_and_across_a_seam():
    """the calm / fast / static sequence of the in-order driver test: with steps of SEQ_STEP frames the oracle's flags take both values inside a chunk and differ
    across a seam"""
    fl = M.seq_flags(); n = len(fl); S = M.SEQ_STEP
    print("sequence flags, frames 1 ..:", " ".join(str(x) for x in fl[1:]))
    assert n == 25 and (n - 1) % S == 0
    chunks = [fl[1 + i:1 + i + S] for i in range(0, n - 1, S)]
    assert 3 <= len(chunks) <= 4
    assert any(set(c) == {0, 1} for c in chunks)
    assert any(chunks[i][-1] != chunks[i + 1][0] for i in range(len(chunks) - 1))
    assert fl[1:] == [0] * 9 + [1] * 7 + [0, 0, 1, 0, 0, 0, 0, 0]
