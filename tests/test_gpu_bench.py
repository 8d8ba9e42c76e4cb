"""bench.py as it is run for every change: a plain run times --steps launches and prints the result line
without the --full legs, and --dump-outputs writes the last step's outputs as float arrays that agree with
the line and with the library called directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import guard_amd
import synth
from rulepack import rule_pack

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_DOCS, N_RES = 300, 8


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--docs", str(N_DOCS), "--resources", str(N_RES), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "(document x rule) evaluations/sec" and line["unit"] == "evals/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["steps"] == 3 and len(line["detail"]["kernel_ms"]) == 3
    ntiles = line["config"]["tiles_per_gpu"]
    assert ntiles == N_DOCS * len(rule_pack("cfg2"))
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(ntiles / (line["ms_per_step"] / 1e3), rel=1e-3)
    # the legs behind --full did not run
    assert line["cpu_baseline"] is None and line["e2e"] is None
    assert not [k for k in line if k.startswith("e2e_") or k == "report_gather"]

    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(arrays) == {"rule_tallies", "tile_counts", "tile_status", "report_sample"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["rule_tallies"].sum() == line["detail"]["rule_tallies_sum"]
    assert list(arrays["tile_counts"]) == line["detail"]["tiles_fail_pass_skip_err"]

    # the same corpus through the library directly: statuses, tallies and the report's bytes
    s = guard_amd.Session()
    for name, text in rule_pack("cfg2"):
        s.add_rules(text, name)
    docs = synth.cfn_corpus(N_DOCS, start=0, n_resources=N_RES)
    s.add_docs(docs, ["synthetic-%d.json" % i for i in range(N_DOCS)])
    s.eval(1)
    assert list(arrays["tile_status"]) == list(s.tile_status(ntiles))
    assert list(arrays["rule_tallies"]) == s.counts()
    text, _ = s.report_range("json", 0, 16)
    assert bytes(arrays["report_sample"].astype(np.uint8)) == text.encode()
    s.close()
