"""The ``--cross-precision`` flag of the two command-line tools (no GPU): ``op`` by default, ``split`` / ``auto`` on request, anything
else refused by the parser."""
import pytest

from mraudio_amd import evaluate, finetune

REQUIRED = {evaluate: ["--output-file", "out/pred.jsonl"], finetune: ["--output-dir", "out/ft", "--dataset", "Charades_STA"]}


@pytest.mark.parametrize("tool", [evaluate, finetune], ids=["evaluate", "finetune"])
def test_cross_precision_flag(tool):
    parser = tool.build_parser()
    assert parser.parse_args(REQUIRED[tool]).cross_precision == "op"
    for mode in ("op", "split", "auto"):
        assert parser.parse_args(REQUIRED[tool] + ["--cross-precision", mode]).cross_precision == mode
    for bad in ("fp32", "AUTO", "2"):
        with pytest.raises(SystemExit):
            parser.parse_args(REQUIRED[tool] + ["--cross-precision", bad])


def test_report_formatting():
    report = {"video": {"mode": "auto", "resolved": "split", "probes": 1, "median_pmax": [0.6, 0.81]},
              "audio": {"mode": "op", "resolved": "op", "probes": 0, "median_pmax": [-1.0, -1.0]}}
    line = evaluate.format_cross_precision(report)
    assert "video: auto -> split (median p_max per cross layer: 0.600, 0.810)" in line
    assert "audio: op -> op (median p_max per cross layer: -)" in line
