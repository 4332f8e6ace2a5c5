"""The CSR chains' look-ahead gathers at engineered reuse distances (tests/reuse_schedule.py).

chain_sparse_lds (HBM tail, fp32 and fp64, SK = 4 and 8) and chain_sparse_spec (SK = 8) read a
row's weights SK samples ahead and repair them through an LDS tag table; chain_sparse and
chain_sparse64 keep the next row's loads in flight. The other CSR tests draw their columns at
random, and their fp32 bar on the folded weights cannot see one stale read late in a chain. Here
every case's rows are built from hazards -- a probe feature at chain positions a and b = a + k and
nowhere between, row b owning a tag column -- at the distances 1..SK+2, around 16, 32, 128, 256,
257..256+SK+1 and 512+k, at every residue of the tagger's step, with the probe in either half of
the row's entries, in runs, at chain ends, in the LDS head as control and spread over the sweep's
chunks (tests/test_reuse_schedule.py audits all that and shows on the CPU that one stale or aliased
read moves row b's tag by more than 4 x the bar).

Each run is one outer iteration under test_gpu_row_coefficients.run_case's checks: the kernel
variant, the chain counts, exact zeros on the tags of rows that were not applied (after the
per-sample break, unsampled), the tag statistic against profiles/row_coefficients.json's BAR /
BAR64 (reused: the restatements' S on these data is within the recorded S_ref, asserted on the
CPU), and the FP32_REL / loss bars (1e-9 in fp64) on the same run. A failure names the hazards that
end at the offending row: chain, positions, distance, feature and entry indices.

The observed statistic of every case goes to the JSON file PSGD_REUSE_SCHEDULE_OUT names
(profiles/reuse_schedule.json's "device" section is one such recording).
"""
import json
import os

import pytest

import reuse_schedule as R
from conftest import has_gpu
from test_gpu_row_coefficients import SPARSE_ENV, describe, run_case

pytestmark = pytest.mark.gpu

RECORD = {}
GPU_CASES = R.gpu_cases()


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not has_gpu():
        pytest.skip("no GPU")
    yield
    out = os.environ.get("PSGD_REUSE_SCHEDULE_OUT")
    if out and RECORD:
        prof = R.load_profile()
        prof["device"] = RECORD
        with open(out, "w") as f:
            json.dump(prof, f, indent=1, sort_keys=True)


def describe_hazard(c, ref, q):
    return f"{describe(c, ref, q)}; {R.describe_hazards(ref, int(ref['which'][q]))}"


@pytest.mark.parametrize("c,want,name", GPU_CASES, ids=[g[2] for g in GPU_CASES])
def test_reuse_schedule(pkg, monkeypatch, c, want, name):
    for k in SPARSE_ENV + ("PSGD_PER_SAMPLE",):
        monkeypatch.delenv(k, raising=False)
    R.build(pkg, c)
    run_case(pkg, monkeypatch, c, want, name, describe=describe_hazard, record=RECORD)
