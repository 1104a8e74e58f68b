"""INTEGRATION.md §5 and the switches csrc/ reads agree (text only, no GPU, no build)."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "miotts-llama.cpp_amd", "csrc")
# a run-time read: the name is the first argument of getenv / env_flag / env_int
READ = re.compile(r'\b(?:getenv|env_flag|env_int)\s*\(\s*"(MIO_[A-Z0-9_]+)"')
# rows the Python binding reads, not csrc/
BINDING_ONLY = {"MIO_BUILD_DIR"}


def _csrc_reads():
    names = set()
    for root, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".cpp", ".h", ".hip")):
                with open(os.path.join(root, f), encoding="utf-8") as fh:
                    names.update(READ.findall(fh.read()))
    return names


def _section5_rows():
    """{name: default cell} of every MIO_* name in the first cell of a §5 table row."""
    with open(os.path.join(REPO, "INTEGRATION.md"), encoding="utf-8") as fh:
        text = fh.read()
    sec = text.split("\n## 5. Environment switches", 1)[1]
    sec = sec.split("\n## ", 1)[0]
    rows = {}
    for line in sec.splitlines():
        if not line.startswith("| `MIO_"):
            continue
        cells = [c.strip() for c in re.split(r"(?<!\\)\|", line)[1:-1]]
        for name in re.findall(r"`(MIO_[A-Z0-9_]+)`", cells[0]):
            rows[name] = cells[1]
    return rows


def test_every_switch_csrc_reads_has_a_row():
    reads, rows = _csrc_reads(), _section5_rows()
    assert reads, "no getenv / env_flag / env_int reads found under csrc/"
    missing = sorted(reads - set(rows))
    assert not missing, f"read in csrc/ but not in INTEGRATION.md §5: {missing}"


def test_every_runtime_row_is_read_in_csrc():
    reads, rows = _csrc_reads(), _section5_rows()
    assert rows, "no rows found in INTEGRATION.md §5"
    stale = sorted(n for n, default in rows.items()
                   if "(compile-time)" not in default and n not in BINDING_ONLY and n not in reads)
    assert not stale, f"INTEGRATION.md §5 rows that csrc/ no longer reads: {stale}"
