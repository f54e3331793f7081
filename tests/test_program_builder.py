"""The compute program builder (csrc/src/program.cpp) without a GPU: a script of the stream's gate-event waits
and records, compute tasks, flushes and the program's end goes in (dlnb_program_script), the task lists the
engine would launch come out. Every expected list is written out by hand from the folding rules: a wait is a
gate of the next task (two slots), a record the done gate of the task right before it, a gate-only task
(flags 1; ticks 1 in a deadline program, 0 in fixed work) carries what fits nowhere, the join tasks take two
gates each, epoch 0, and the last one stores the done word."""
import pytest

from dlnetbench_amd import _native


def task(epoch, ticks=0, gates=(0, 0, 0, 0), done=(0, 0), flags=0, rounds=0, tail=0, tstart=(0, 0), gate_timeout=60):
    """One task as dlnb_program_script prints it: gates = (gate0, tag0, gate1, tag1), done = (gate, tag),
    base = the iter / counters / abort words are the engine's."""
    return {"ticks": ticks, "epoch": epoch, "rounds": rounds, "tail": tail, "flags": flags, "gates": list(gates),
            "done": list(done), "tstart": list(tstart), "gate_timeout": gate_timeout, "base": True}


def gate_only(epoch, gates=(0, 0, 0, 0), done=(0, 0), ticks=1, **kw):
    return task(epoch, ticks=ticks, gates=gates, done=done, flags=1, **kw)


def run(script, fixed_work=False):
    return _native.program_script("\n".join(script), fixed_work)


def test_waits_become_gates():
    doc = run(["begin", "wait 1 5", "wait 2 6", "task 500", "end 0"])
    assert doc == {"launches": [[task(0, 500, gates=(1, 5, 2, 6))]], "joined": False}


def test_a_third_wait_spills_into_a_gate_only_task():
    doc = run(["begin", "wait 1 1", "wait 2 2", "wait 3 3", "task 500", "end 0"])
    assert doc["launches"] == [[gate_only(0, gates=(1, 1, 0, 0)), task(1, 500, gates=(2, 2, 3, 3))]]


def test_a_task_with_a_gate_of_its_own_keeps_it_in_slot_0():
    doc = run(["begin", "wait 1 1", "wait 2 2", "task 500 0 0 5 9", "end 0"])
    assert doc["launches"] == [[gate_only(0, gates=(1, 1, 0, 0)), task(1, 500, gates=(5, 9, 2, 2))]]


def test_the_same_gate_waited_twice_keeps_its_latest_tag():
    doc = run(["begin", "wait 1 1", "wait 1 4", "task 500", "end 0"])
    assert doc["launches"] == [[task(0, 500, gates=(1, 4, 0, 0))]]


def test_records_after_a_task():
    # the first record right after the task is its done gate; the second finds that taken: a gate-only task
    doc = run(["begin", "task 500", "record 7 2", "end 0"])
    assert doc["launches"] == [[task(0, 500, done=(7, 2))]]
    doc = run(["begin", "task 500", "record 7 2", "record 8 1", "end 0"])
    assert doc["launches"] == [[task(0, 500, done=(7, 2)), gate_only(1, done=(8, 1))]]


def test_a_record_with_three_waits_pending():
    doc = run(["begin", "task 500", "wait 1 1", "wait 2 2", "wait 3 3", "record 9 1", "end 0"])
    assert doc["launches"] == [[task(0, 500), gate_only(1, gates=(1, 1, 2, 2)),
                                gate_only(2, gates=(3, 3, 0, 0), done=(9, 1))]]


def test_a_record_as_the_first_thing():
    doc = run(["begin", "record 9 1", "end 0"])
    assert doc["launches"] == [[gate_only(0, done=(9, 1))]]


def test_flush():
    doc = run(["begin", "task 500", "wait 1 1", "flush", "record 2 1", "task 600", "end 0",
               "begin", "task 700", "end 0"])
    assert doc["launches"] == [
        [task(0, 500), gate_only(1, gates=(1, 1, 0, 0))],  # the pending wait leaves with the launch
        [gate_only(2, done=(2, 1)), task(3, 600)],         # no task left to take the record; the index runs on
        [task(0, 700)],                                    # a new program restarts it
    ]


def test_join_of_three_gates():
    doc = run(["begin", "task 500", "join 50 1 1 2 3", "end 1"])
    assert doc == {"launches": [[task(0, 500), task(0, gates=(1, 1, 2, 1)),
                                 task(0, gates=(3, 1, 0, 0), tstart=(50, 0))]], "joined": True}


def test_join_with_no_gates():
    doc = run(["begin", "task 500", "join 50 1", "end 1"])
    assert doc == {"launches": [[task(0, 500), task(0, tstart=(50, 0))]], "joined": True}


def test_join_follows_the_waits_after_the_last_task():
    doc = run(["begin", "task 500", "wait 4 2", "join 50 1 1", "end 1"])
    assert doc["launches"] == [[task(0, 500), gate_only(1, gates=(4, 2, 0, 0)),
                                task(0, gates=(1, 1, 0, 0), tstart=(50, 0))]]


def test_join_refused():
    doc = run(["begin", "task 500", "join 50 1 1 2 3", "end 0"])
    assert doc == {"launches": [[task(0, 500)]], "joined": False}


def test_join_on_an_empty_program():
    doc = run(["begin", "task 500", "join 50 1 1", "flush", "end 1"])
    assert doc == {"launches": [[task(0, 500)], []], "joined": False}


def test_fixed_work_gate_only_tasks_have_no_ticks():
    doc = run(["begin", "wait 1 1", "wait 2 2", "wait 3 3", "task 0 2 4", "record 7 1", "record 8 1", "end 0"],
              fixed_work=True)
    assert doc["launches"] == [[gate_only(0, gates=(1, 1, 0, 0), ticks=0),
                                task(1, rounds=2, tail=4, gates=(2, 2, 3, 3), done=(7, 1)),
                                gate_only(2, done=(8, 1), ticks=0)]]


def test_gate_timeout_set_later_reaches_the_tasks_built_after_it():
    doc = run(["begin", "task 500", "wait 1 1", "flush", "timeout 99", "wait 2 1", "join 50 1", "end 1"])
    assert doc["launches"] == [[task(0, 500), gate_only(1, gates=(1, 1, 0, 0))],
                               [gate_only(2, gates=(2, 1, 0, 0), gate_timeout=99),
                                task(0, tstart=(50, 0), gate_timeout=99)]]


def test_task_limit():
    doc = run(["begin"] + ["task 500"] * 4096 + ["end 0"])
    assert [t["epoch"] for t in doc["launches"][0]] == list(range(4096))
    with pytest.raises(_native.NativeError, match="more than 4096 program tasks per iteration on one stream"):
        run(["begin"] + ["task 500"] * 4097)
    # a gate-only task counts like any other
    with pytest.raises(_native.NativeError, match="more than 4096 program tasks per iteration on one stream"):
        run(["begin"] + ["task 500"] * 4096 + ["wait 1 1", "flush"])


def test_begin_twice():
    with pytest.raises(_native.NativeError, match="begin_program: a program is already open on this stream"):
        run(["begin", "begin"])
