"""The randomised differential test of whole sessions of one context (tests/fuzz_sessions.py) as part of the `-m gpu` suite: a fixed
schedule of sessions of 5 to 7 batches of different content and size through ONE context each, in groups of up to SHK_PIPE_DEPTH tickets
in flight (host and resident tickets mixed), with mode switches, resets, changes of kind, a replaced site list, shk_pileup_add and
shk_indels_add between the groups.  After every wait that hand-out's records are compared byte for byte with its own batch's models,
after every group every accumulated state element for element with the running sum of the models -- the states whose mode is off at
that moment too.  No tolerances.

tests/test_fuzz_sessions_cpu.py asserts, with the models alone, what this schedule covers and that the comparison sees the faults it is
there for; the last test here asserts on the device that both repair paths ran INSIDE sessions and that every entry family ran.

Measured on an MI355X: MEASURED below.

Run on the GPU box with `pytest -m gpu`."""
import pytest

from tests import fuzz_sessions as fs

pytestmark = pytest.mark.gpu

# chosen with the models alone until tests/test_fuzz_sessions_cpu.py's coverage conditions held; a session's flavour is FLAVOURS[seed % 4],
# and the `overflow` ones (a batch of 700 pairs tied over twelve records: 8 400 associations through every model) run one per test
SEEDS = [20340021, 20340025, 20340026, 20340028, 20340032, 20340033, 20340036, 20340037, 20340039, 20340040, 20340043, 20340044, 20340047, 20340049,
         20340052]
# MEASURED on an MI355X, in one run of the whole suite, the file's share as the sum of its tests: 29 s of 784 s (10 of 1 335 tests; the suite
# without this file 755 s in that run, and this file alone, in a run of its own, 30.3 s): the three overflow sessions 5.5, 4.6 and 2.7 s,
# every pair of other sessions under 4.0 s, most of it the models on the CPU.  tests/test_gpu_fuzz_records.py was measured at 31.6 s of
# 765 s: the file adds about 4 % to the suite, as that one does

CHUNKS, _pair = [], []
for _seed in SEEDS:
    if fs.FLAVOURS[_seed % len(fs.FLAVOURS)] == "overflow":
        CHUNKS.append((_seed,))
    else:
        _pair.append(_seed)
        if len(_pair) == 2:
            CHUNKS.append(tuple(_pair))
            _pair = []
if _pair:
    CHUNKS.append(tuple(_pair))
FACTS = {}       # seed -> per step what run_session reports and what the model expected, for the last test


def run_one(oracle, seed):
    if seed not in FACTS:
        session = fs.draw_session(seed)
        want = fs.expected_session(session, oracle)
        bad, facts = fs.run_session(session, oracle, want)
        assert not bad, "MISMATCH: %s\n%s" % (fs.describe_session(session), bad)
        for f, w, slot in zip(facts, want["steps"], want["slots"]):
            f.update(expect_long=w["expect_long"], expect_overflow=slot["overflow"], cap=slot["cap"], indels=w["expect_indels"])
        FACTS[seed] = facts
    return FACTS[seed]


@pytest.mark.parametrize("seeds", CHUNKS, ids=lambda seeds: "-".join(str(s) for s in seeds))
def test_fuzz_sessions(oracle, seeds):
    for seed in seeds:
        run_one(oracle, seed)


def test_schedule_ran_both_repair_paths_inside_sessions_and_every_family(oracle):
    """tests/test_gpu_fuzz_records.py's last test for sessions: where the model expected it behind a session's first step, the length-bound
    repair ran (a resident ticket behind a bound that does not hold: timing()["last_n_long"] > 0 behind its wait) and the overflow repair
    ran (more associations handed out than the slot's reservation held, as the slot had grown by then) -- each with indels mode on, the
    record arrays holding other batches' records --, and every entry family ran"""
    facts = [f for seed in SEEDS for f in run_one(oracle, seed)]
    long_steps = [f for f in facts if f["expect_long"] and f["family"] == "submit_device" and f["step"] > 0]
    assert len(long_steps) >= 3 and all(f["last_n_long"] > 0 for f in long_steps), [(f["family"], f["last_n_long"]) for f in long_steps]
    over = [f for f in facts if f["expect_overflow"] and f["step"] > 0]
    assert len(over) >= 3 and all(f["n_assoc"] > f["cap"] for f in over), [(f["n_assoc"], f["cap"]) for f in over]
    assert any(f["indels"] for f in over) and any(f["indels"] for f in long_steps)
    assert {f["family"] for f in facts} == set(fs.fz.FAMILIES)
    print("fuzz sessions: %d sessions, %d steps" % (len(SEEDS), len(facts)))
