"""CPU: the whole usage surface of the `distance` CLI against the recorded outcomes of tests/cli_usage_outcomes.json
(tools/record_cli_usage.py, from the commit the fixture names): every subset of up to three of 26 argument groups, and
every value word for every flag that takes one (tests/cli_usage_cases.py).  A case's exit code, the length of its stdout
and the first line of its stderr must all be the recorded ones, so a rewritten parse_args names the same flag, from the
same mode, in the same order as the one the fixture was recorded from."""
import json
import os
import subprocess

import pytest

import cli_usage_cases as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")
FIXTURE = os.path.join(ROOT, "tests", "cli_usage_outcomes.json")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_case_list_is_the_recorded_one(fixture):
    case_list = cu.cases()
    assert len(cu.subset_cases()) == 2927
    assert len(case_list) == fixture["n_cases"] == len(fixture["cases"])
    assert cu.cases_digest(case_list) == fixture["cases_sha256"]


def test_fixture_stays_small():
    assert os.path.getsize(FIXTURE) < 100_000


def test_every_case_has_its_recorded_outcome(fixture):
    case_list = cu.cases()
    want = cu.unpack(fixture)
    got = cu.run_all(CLI, case_list)
    assert len(got) == len(want) == len(case_list)
    wrong = [(args, w, g) for args, w, g in zip(case_list, want, got) if w != g]
    assert not wrong, f"{len(wrong)} of {len(case_list)} cases differ; the first: " + "; ".join(
        f"{' '.join(args)}: recorded {w}, now {g}" for args, w, g in wrong[:5])
