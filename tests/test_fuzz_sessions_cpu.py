"""The session fuzz (tests/fuzz_sessions.py) without a GPU: draw_session and expected_session over the schedule
tests/test_gpu_fuzz_sessions.py commits, with the models alone.  Asserted: the generator is deterministic and leaves the record fuzz's
random streams alone; every session is legal by the header's rules and has the shape it is drawn for; the schedule COVERS what it was
chosen for (every fact below at least three times); a faultless device passes; and the comparison REPORTS each of the faults it is
there for, planted into results made from the model -- a driver that cannot see these proves nothing on the device:

  (a) the records of two tickets of one group swapped (whole hand-outs, and the records alone behind the right associations)
  (b) one step's contribution missing from one accumulator, each of the five in turn
  (c) a reset that was not applied
  (d) the records of the slot's earlier, larger batch behind the current batch's last association counted into depth, pileup and the
      indel table
  (e) a mode that was off for a group counted anyway

Measured here (CPU): TIMING below."""
import collections

import numpy as np
import pytest

from tests import fuzz_records as fz
from tests import fuzz_sessions as fs
from tests.indels_model import table_array
from tests.test_gpu_fuzz_sessions import CHUNKS, SEEDS

# TIMING: the whole file takes about 77 s on the CPU it was written on: the schedule's 15 sessions (89 steps) 63 s, among them the three
# overflow batches of 700 pairs tied over twelve records about 25 s; the planted faults 12 s, most of it fault (e)'s and (d)'s extra models

AT_LEAST = 3
FACTS = (
    ["group.2", "group.3", "group.mixed", "slot_grown", "seg_m.4_below_4", "launches.three", "sites_replaced.changes_a_record", "paired_single_paired",
     "repair.overflow.inside", "repair.length.inside", "repair.length.inside.submit_device", "pileup_add", "indels_add"]
    + ["fewer_in_slot." + kind for kind in fs.STATE_KINDS] + ["off_on." + kind for kind in fs.STATE_KINDS]
    + ["launches.%s.%s" % (what, how) for what in ("pileup", "indels") for how in ("merged", "split")]
    + ["reset." + s for s in fs.STATES] + ["kind_after_reset." + s for s in fs.STATES] + ["family." + f for f in fz.FAMILIES]
)
NAMES = {"depth": "depth", "junctions": "junction table", "pileup": "pileup", "fragments": "fragment", "indels": "indel"}      # as check_states reports them


@pytest.fixture(scope="module")
def sessions(oracle):
    """[(session, expected)] over the schedule, computed once"""
    out = []
    for seed in SEEDS:
        session = fs.draw_session(seed)
        out.append((session, fs.expected_session(session, oracle)))
    return out


def group_of(session, i):
    return session["steps"][i]["group"]


def with_states(session, want, snapshots):
    """a faultless device's results with the states replaced"""
    results = fs.model_results(session, want)
    results["states"] = [{key: v for key, v in snap.items() if key != "empty"} for snap in snapshots]
    return results


def test_draw_session_is_deterministic_and_leaves_the_record_fuzz_alone():
    for seed in (SEEDS[0], SEEDS[-1]):
        a, b = fs.draw_session(seed), fs.draw_session(seed)
        assert fs.describe_session(a) == fs.describe_session(b) and a["sites"] == b["sites"]
        assert [bytes(r) for r in a["records"]] == [bytes(r) for r in b["records"]]
        for s, t in zip(a["steps"], b["steps"]):
            assert s["calls"] == t["calls"] and s["modes"] == t["modes"] and (s["family"], s["bound"], s["slot"]) == (t["family"], t["bound"], t["slot"])
            assert all((s["batch"][x] is None and t["batch"][x] is None) or s["batch"][x].tobytes() == t["batch"][x].tobytes() for x in s["batch"])
    assert fs.draw_session(SEEDS[0])["steps"][0]["batch"]["seq1"].tobytes() != fs.draw_session(SEEDS[0] + 4)["steps"][0]["batch"]["seq1"].tobytes()
    # a stream of its own: no (seed, key) pair of tests/fuzz_records.py's draws is [seed, SESSION_KEY]
    assert fs.SESSION_KEY not in set(fz.BIAS_KEY.values()) | {fz.WIDE_B_KEY, fz.WIDE_C_KEY}


def test_every_session_is_legal_and_has_its_shape(sessions):
    """the header's rules, walked over the drawn calls: calls only in front of a group; at most SHK_PIPE_DEPTH tickets per group, every
    one another batch; sizes from the issue's set; a state takes another kind, capacity, n_bins or min_intron only while it holds nothing;
    pairs and rescue mode are switched on only while alignments mode is on; and the two reuses every session is drawn for are there"""
    assert len(CHUNKS) >= 1 and sorted(s for c in CHUNKS for s in c) == sorted(SEEDS) and len(set(SEEDS)) == len(SEEDS)
    for session, want in sessions:
        steps = session["steps"]
        assert 4 <= len(steps) <= 7 and all(s["n"] in fs.SIZES and s["n"] <= 700 for s in steps), fs.describe_session(session)
        assert all(len(idx) <= fz.capi.SHK_PIPE_DEPTH for idx in want["groups"])
        assert all(len(idx) == 1 or all(steps[i]["family"] in ("submit", "submit_device") for i in idx) for idx in want["groups"])
        assert all(not steps[i]["calls"] for idx in want["groups"] for i in idx[1:])
        assert len({s["batch"]["seq1"].tobytes() for s in steps}) == len(steps)
        turning = [s["slot"] for s in steps if s["family"] != "classify_device"]
        assert turning == [r % fz.capi.SHK_PIPE_DEPTH for r in range(len(turning))]
        assert all(s["slot"] == fz.capi.SHK_PIPE_DEPTH for s in steps if s["family"] == "classify_device")
        assert all(s["bound"] > 0 and s["bound"] <= fz.largest_submit_bound(session["k"], s["paired"]) for s in steps if s["family"] == "submit_device")
        assert want["coverage"].get("fewer_in_slot", 0) >= 1 and want["coverage"].get("slot_grown", 0) >= 1, fs.describe_session(session)
        dirty = {s: None for s in fs.STATES}
        al = 0
        shape = {"junctions": None, "fragments": None, "indels": None}
        for i, s in enumerate(steps):
            for name, args in s["calls"]:
                if name.endswith("_reset"):
                    dirty[name[:-6]] = None
                elif name in ("depth_enable", "depth_enable_spliced") and args[0]:
                    assert dirty["depth"] in (None, "plain" if name == "depth_enable" else "spliced"), (fs.describe_session(session), i, name)
                elif name in ("pileup_enable", "pileup_enable_aligned") and args[0]:
                    assert dirty["pileup"] in (None, True, "owned" if name == "pileup_enable" else "aligned"), (fs.describe_session(session), i, name)
                elif name == "junctions_enable" and args[0]:
                    assert not dirty["junctions"] or shape["junctions"] == args[1], (fs.describe_session(session), i, name)
                    shape["junctions"] = args[1]
                elif name == "indels_enable" and args[0]:
                    assert not dirty["indels"] or shape["indels"] == args[1:], (fs.describe_session(session), i, name)
                    assert 1 <= args[1] <= 65535
                    shape["indels"] = args[1:]
                elif name == "alignments_enable":
                    al = args[0]
                elif name == "pairs_enable" and args[2]:
                    assert al and (not dirty["fragments"] or shape["fragments"] == args[2]), (fs.describe_session(session), i, name)
                    shape["fragments"] = args[2]
                elif name == "rescue_enable" and args[1]:
                    assert al and 1 <= args[1] <= 4096
                elif name in ("pileup_add", "indels_add"):
                    assert args[0] < i and steps[args[0]]["modes"][name[:-4]]
                    dirty[name[:-4]] = dirty[name[:-4]] or True
            md = s["modes"]
            assert al == md["al_floor"] and shape["fragments"] == s["n_bins"]
            if md["depth"]:
                dirty["depth"] = md["depth"][0]
            if md["pileup"]:
                assert dirty["pileup"] in (None, True, md["pileup"][0])
                dirty["pileup"] = md["pileup"][0]
            dirty["junctions"] = dirty["junctions"] or bool(md["junc_floor"])
            dirty["fragments"] = dirty["fragments"] or bool(md["al_floor"] and md["pairs"])
            dirty["indels"] = dirty["indels"] or bool(md["indels"])


def test_the_schedule_covers_every_fact(sessions):
    total = collections.Counter()
    for _, want in sessions:
        total.update(want["coverage"])
    print("coverage over %d sessions, %d steps: %s" % (len(sessions), sum(len(s["steps"]) for s, _ in sessions), dict(sorted(total.items()))))
    missing = {f: total[f] for f in FACTS if total[f] < AT_LEAST}
    assert not missing, "met fewer than %d times: %s" % (AT_LEAST, missing)
    # the overflow repair inside a session is the slot's GROWN reservation exceeded, at no more than 700 pairs
    over = [(s["steps"][i], w["steps"][i], w["slots"][i]) for s, w in sessions for i in range(len(s["steps"])) if w["slots"][i]["overflow"]]
    assert all(step["n"] <= 700 and int(w["goff"][-1]) > slot["cap"] >= fz.slot_reserve(step["n"]) and slot["held"] is not None for step, w, slot in over)


def test_a_faultless_device_passes_and_the_fold_is_the_model(sessions):
    for session, want in sessions:
        assert fs.check_session(session, want, fs.model_results(session, want)) is None
    session, want = sessions[0]
    assert fs.check_session(session, want, with_states(session, want, fs.fold_states(session, want["steps"]))) is None


def test_fault_a_two_tickets_of_a_group_swapped(sessions):
    seen = 0
    for session, want in sessions:
        for idx in want["groups"]:
            if len(idx) < 2:
                continue
            i, j = idx[0], idx[-1]
            results = fs.model_results(session, want)
            results["hand_outs"][i], results["hand_outs"][j] = results["hand_outs"][j], results["hand_outs"][i]
            said = fs.check_session(session, want, results)
            assert said and said.startswith("step %d " % i), (fs.describe_session(session), i, j, said)
            # the associations right and the records the other ticket's: what a wrong slot's mirror behind the right result would show
            results = fs.model_results(session, want)
            (gi, di, ri), (gj, dj, rj) = results["hand_outs"][i], results["hand_outs"][j]
            if set(ri) == set(rj) and int(gi[-1]) + int(gj[-1]) > 0:
                results["hand_outs"][i], results["hand_outs"][j] = (gi, di, rj), (gj, dj, ri)
                said = fs.check_session(session, want, results)
                assert said and said.startswith("step %d " % i) and "gene_" not in said, (fs.describe_session(session), i, j, said)
                seen += 1
    assert seen >= 10


def test_fault_b_a_step_missing_from_an_accumulator(sessions):
    seen = collections.Counter()
    for session, want in sessions:
        for i, w in enumerate(want["steps"]):
            for state in fs.STATES:
                gives = {"depth": lambda: w["depth"][1], "junctions": lambda: len(w["junctions"]), "pileup": lambda: w["pileup"][1],
                         "fragments": lambda: int(w["fragments"][1].sum()), "indels": lambda: w["indels"][1]["mates"]}
                if state not in w or not gives[state]() or seen[state] >= 4:
                    continue
                said = fs.check_session(session, want, with_states(session, want, fs.fold_states(session, want["steps"], skip={(i, state)})))
                assert said and said.startswith("behind group %d " % group_of(session, i)) and ": " + NAMES[state] in said, (state, i, said)
                seen[state] += 1
    assert all(seen[state] >= 3 for state in fs.STATES), seen


def test_fault_c_a_reset_not_applied(sessions):
    """(not the fragments reset in front of another n_bins: that state is allocated anew, reset or not)"""
    seen = collections.Counter()
    for session, want in sessions:
        for i, s in enumerate(session["steps"]):
            for j, (name, _) in enumerate(s["calls"]):
                if name == "fragments_reset" and s["n_bins"] != session["steps"][i - 1]["n_bins"]:
                    continue
                if i and name.endswith("_reset") and not want["snapshots"][group_of(session, i) - 1]["empty"][name[:-6]] and seen[name] < 3:
                    said = fs.check_session(session, want, with_states(session, want, fs.fold_states(session, want["steps"], unapplied={(i, j)})))
                    assert said and said.startswith("behind group %d " % group_of(session, i)) and ": " + NAMES[name[:-6]] in said, (name, i, said)
                    seen[name] += 1
    assert all(seen[s + "_reset"] >= 2 for s in fs.STATES), seen


def contribution(w, minus=None):
    """a step's contribution to depth, pileup and the indel table in fuzz_records.expected's form; minus: another's taken off it"""
    out = {}
    if minus is None:
        return {key: w[key] for key in ("depth", "pileup", "indels") if key in w}
    for key in ("depth", "pileup"):
        if key in w:
            out[key] = (w[key][0] - minus[key][0], int(w[key][1]) - int(minus[key][1]))
    if "indels" in w:
        table = {tuple(int(e[f]) for f in ("gene", "x", "kind", "len", "seq")): [int(e["fwd"]), int(e["rev"])] for e in w["indels"][0]}
        for e in minus["indels"][0]:
            t = table[tuple(int(e[f]) for f in ("gene", "x", "kind", "len", "seq"))]
            t[0], t[1] = t[0] - int(e["fwd"]), t[1] - int(e["rev"])
        out["indels"] = (table_array({key: v for key, v in table.items() if v[0] or v[1]}), {name: v - minus["indels"][1][name] for name, v in w["indels"][1].items()})
    return out


def test_fault_d_the_slots_earlier_records_counted(sessions, oracle):
    """a slot's record arrays hold the earlier, larger batch's records behind the current batch's last association.  What a kernel with a
    bound off by the whole tail would add: the earlier batch's contribution less that of its reads in front of the bound -- the model over
    the same batch with the reads from there on emptied (a read's associations and records are its own)"""
    seen = 0
    for session, want in sessions:
        steps = session["steps"]
        for j, slot in enumerate(want["slots"]):
            p = max((i for i in range(j) if steps[i]["slot"] == steps[j]["slot"]), default=None)
            if p is None or seen >= 3:
                continue
            wp, n_now = want["steps"][p], int(want["steps"][j]["goff"][-1])
            if not (n_now < int(wp["goff"][-1]) <= 3000 and all(key in wp and key in want["steps"][j] for key in ("depth", "pileup", "indels"))):
                continue
            keep = int(np.searchsorted(wp["goff"], n_now, side="left"))          # the first read whose records lie behind the bound
            front = fz.expected(fs.step_case(session, steps[p], batch=fz.emptied_from(steps[p]["batch"], keep)), oracle, primed=False)
            stale = contribution(wp, minus=front)
            if not (stale["depth"][1] and stale["pileup"][1] and stale["indels"][1]["mates"] and len(stale["indels"][0])):
                continue
            for keys in (("depth", "pileup", "indels"), ("depth",), ("pileup",), ("indels",)):
                extra = {j: {key: stale[key] for key in keys}}
                said = fs.check_session(session, want, with_states(session, want, fs.fold_states(session, want["steps"], extra=extra)))
                assert said and said.startswith("behind group %d " % group_of(session, j)) and ": " + NAMES[keys[0]] in said, (keys, j, said)
            seen += 1
    assert seen >= 2


def test_fault_e_a_mode_that_was_off_counted_anyway(sessions, oracle):
    seen = collections.Counter()
    for session, want in sessions:
        steps = session["steps"]
        for g in range(1, len(want["groups"])):
            i = want["groups"][g][0]
            was, now = steps[want["groups"][g - 1][0]]["modes"], steps[i]["modes"]
            for state, keys in (("depth", ("depth",)), ("junctions", ("junc_floor",)), ("pileup", ("pileup",)), ("indels", ("indels",)), ("fragments", ("al_floor", "pairs"))):
                off = not all(now[k] for k in keys) and all(was[k] for k in keys)
                if not off or seen[state] >= 2 or int(want["steps"][i]["goff"][-1]) > 3000:
                    continue
                on = fz.expected(fs.step_case(session, steps[i], modes=dict(now, **{k: was[k] for k in keys})), oracle, primed=False)
                if state not in on or not {"depth": lambda: on["depth"][1], "junctions": lambda: len(on["junctions"]), "pileup": lambda: on["pileup"][1],
                                           "indels": lambda: on["indels"][1]["mates"], "fragments": lambda: int(on["fragments"][1].sum())}[state]():
                    continue
                said = fs.check_session(session, want, with_states(session, want, fs.fold_states(session, want["steps"], extra={i: {state: on[state]}})))
                assert said and said.startswith("behind group %d " % g) and ": " + NAMES[state] in said, (state, i, said)
                seen[state] += 1
    assert sum(seen.values()) >= 5 and len(seen) >= 4, seen
