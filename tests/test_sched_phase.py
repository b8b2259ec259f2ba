"""CPU check of option "reorder"'s schedule decision (csrc/sched_phase.hpp, which rt_render's schedule step calls):
tests/cpp/sched_phase_check.cpp, built with the address and undefined-behaviour sanitizers and run as a process of
its own, compares sched_step with the branch it replaced for every (layout_ok, K, phase), and walks 3 K launches of
one lane from a fresh layout."""
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sched_phase") / "sched_phase_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "cpp", "sched_phase_check.cpp")], check=True)
    return exe


def _run(checker, *args):
    p = subprocess.run([checker, *args], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout)


def test_decision_equals_the_branch_it_replaced(checker):
    r = _run(checker, "table")
    # layout_ok x (K = 1..9, phase < K: 45 pairs) x the lane's order flag before the launch
    assert r["cases"] == 2 * 45 * 2 and r["mismatches"] == 0, r


@pytest.mark.parametrize("K", [1, 2, 8])
def test_walk_from_a_fresh_layout(checker, K):
    r = _run(checker, "walk", str(K))
    assert r["first_records_in_screen_order"] == 1, r
    assert r["stale_orders"] == 0 and r["orders_without_schedule"] == 0, r
    assert r["bad_periods"] == 0, r
    # 3 K launches: K = 1 records on every launch and orders on all but the first; else the first launch records, the
    # second orders, and each later period of K launches holds one of each
    assert r["records"] == 3 and r["orders"] == (2 if K == 1 else 3), r
