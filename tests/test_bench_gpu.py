"""A plain bench.py run on the device: the headline line and the last step's outputs, and none of
what --full adds (other configs, CPU baseline)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

pytestmark = pytest.mark.gpu


def test_plain_run_reports_only_the_headline(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--N", "256",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    rec = json.loads(line[0])
    assert rec["unit"] == "utterances/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(256 * 1e3 / rec["ms_per_step"])
    assert not {"other_configs", "config_summary", "cpu_baseline"} & set(rec)
    assert sorted(p.name for p in out.iterdir()) == sorted(
        n + ".npy" for n in ("error_rate", "prefix_error_rates", "optimal_completion", "ctc_prefix_search_y",
                             "ctc_prefix_search_y_lens", "ctc_prefix_search_y_probs"))
