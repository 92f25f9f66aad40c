"""Completeness guard of tests/test_gpu_streams.py (no GPU): every prototype of include/lm_engine.h and include/lm_policy.h that takes a
`void* stream` is named in that module's COVERED table, with the cases that run it on a caller's stream.  An entry point added later without a
stream case fails here."""
import os
import re

from conftest import ROOT

import test_gpu_streams as S


def stream_prototypes():
    names = set()
    for header in ("lm_engine.h", "lm_policy.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)          # the comments quote prototypes too
        for m in re.finditer(r"\b(lm_\w+)\s*\(([^;{}]*?)\)\s*;", text):
            if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
                names.add(m.group(1))
    return names


def test_the_headers_are_parsed():
    """A few prototypes of either kind, so that a parser that finds nothing cannot pass the guard."""
    names = stream_prototypes()
    assert {"lm_step", "lm_rollout_run", "lm_ppo_batch_apply", "lm_mlp_forward", "lm_debug_dynamics"} <= names
    assert not names & {"lm_create", "lm_set_env_params", "lm_rollout_create", "lm_rollout_set_trajectory_record", "lm_ptr"}
    assert len(names) >= 26


def test_every_stream_entry_point_has_a_case():
    names = stream_prototypes()
    assert names == set(S.COVERED), {"without a stream case": sorted(names - set(S.COVERED)), "not in the headers": sorted(set(S.COVERED) - names)}
    assert all(S.COVERED[n] for n in names)


def test_covered_names_cases_that_exist():
    """Every id in COVERED is a case of test_on_a_callers_stream or a test function of the module, and every case is listed."""
    listed = {c for ids in S.COVERED.values() for c in ids}
    cases = {c for c in listed if not c.startswith("test_")}
    assert cases == set(S.CASES), {"unknown": sorted(cases - set(S.CASES)), "unlisted": sorted(set(S.CASES) - cases)}
    for t in listed - cases:
        assert callable(getattr(S, t, None)), t
