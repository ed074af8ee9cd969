"""The documents against the committed measurements and the tree (CPU).

DESIGN.md / README.md / INTEGRATION.md / scripts/README.md quote numbers from `profiles/` and name
files of this repository.  These checks keep them from drifting: every repository file they name
exists, README's headline is the committed headline bench line, and DESIGN §5's configuration table
is the committed reconciliation (`profiles/round6/roofline_reconcile.json`)."""
from __future__ import annotations

import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = ["DESIGN.md", "README.md", "INTEGRATION.md", os.path.join("scripts", "README.md")]
ROUND = os.path.join(ROOT, "profiles", "round6")

# names of the reference's own sources (in /root/reference, cited by file:line) and of files a
# document says are gone
NOT_OURS = {"cnode.cpp", "utils.cpp", "cnode.h", "cytree.pyx", "ctree.pxd", "mazero_amd/_hipenv.py"}
# per-configuration files of profiles/<round>/<config>/
PER_CONFIG = {"bench.json", "traced.json", "pmc_summary.txt", "rocprof_kernel_stats.csv",
              "rocprof_timed_window.json"}


def _read(doc: str) -> str:
    with open(os.path.join(ROOT, doc)) as f:
        return f.read()


@pytest.mark.parametrize("doc", DOCS)
def test_named_files_exist(doc):
    text = _read(doc)
    names = set(re.findall(r"`([A-Za-z0-9_./-]+\.(?:py|sh|hip|json|jsonl|md|h|cpp|log|npz|txt|csv))`", text))
    missing = []
    for n in sorted(names):
        if n in NOT_OURS or n.startswith(("core/", "common_lib/", "config/")) or os.path.basename(n) in NOT_OURS:
            continue
        if n in PER_CONFIG:
            assert os.path.exists(os.path.join(ROUND, "3m_k1", n)), n
            continue
        cands = [n] + [os.path.join(d, n) for d in ("scripts", "mazero_amd", "mazero_amd/csrc", "oracle", "include",
                                                     "tests", "profiles/round6", "profiles/round6/ab", "profiles/round5", "profiles/round4", "profiles/round3",
                                                     "profiles")]
        if not any(os.path.exists(os.path.join(ROOT, c)) for c in cands):
            missing.append(n)
    assert not missing, f"{doc} names files that do not exist: {missing}"


def test_build_switches_are_the_documented_ones():
    """Every MZ_* name a preprocessor conditional of the kernel sources tests is a row of DESIGN §3's
    compile-time switch table, and the other way round: a new knob has to be documented."""
    csrc = os.path.join(ROOT, "mazero_amd", "csrc")
    used = set()
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".inc", ".h")):
            continue
        with open(os.path.join(csrc, name)) as f:
            text = re.sub(r"\\[ \t]*\n", " ", f.read())  # a directive continued with a backslash is one line
        for line in text.splitlines():
            m = re.match(r"\s*#\s*(ifdef|ifndef|if|elif)\b(.*)", line)
            if m:
                cond = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
                used |= set(re.findall(r"\bMZ_[A-Z0-9_]+\b", cond))
    text = _read("DESIGN.md")
    sec = text[text.index("### Build switches"):text.index("## 4. Parity and the oracle")]
    table = sec[sec.index("| Compile-time switch |"):sec.index("| Run-time flag")]
    listed = set(re.findall(r"^\| `(MZ_[A-Z0-9_]+)` \|", table, flags=re.M))
    assert listed, "DESIGN §3's compile-time switch table"
    assert used == listed, (sorted(used - listed), sorted(listed - used))


def _bench(config: str) -> dict:
    with open(os.path.join(ROUND, config, "bench.json")) as f:
        return json.loads(f.readline())


def test_readme_headline_is_the_committed_line():
    b = _bench("3m_k1")
    m = re.search(r"\*\*([0-9.]+) M\s+simulations/s\*\*", _read("README.md"))
    assert m, "README's headline sentence"
    assert abs(float(m.group(1)) - b["value"] / 1e6) < 0.05
    cpu = b["cpu_baseline"]["value"]
    r = re.search(r"([0-9,]+)×\s+the reference ctree on one host core", _read("README.md"))
    assert r and abs(int(r.group(1).replace(",", "")) - b["value"] / cpu) <= 1


def test_design_table_is_the_committed_reconciliation():
    with open(os.path.join(ROUND, "roofline_reconcile.json")) as f:
        rec = json.load(f)
    rows = {}
    text = _read("DESIGN.md")
    sec = text[text.index("### Round 6 (`profiles/round6/`)"):text.index("### Round 5 (for the record")]
    for line in sec.splitlines():
        m = re.match(r"\| (3m|2s3z|3s5z_vs_3s6z|27m_vs_30m) (\d+)×(\d+) K=(\d+) \| ([0-9.]+) M \| [^|]+\| ([0-9.]+) µs \|",
                     line)
        if m:
            key = {"3m": "3m", "2s3z": "2s3z", "3s5z_vs_3s6z": "3s5z", "27m_vs_30m": "27m"}[m.group(1)] + f"_k{m.group(4)}"
            rows[key] = (float(m.group(5)), float(m.group(6)))
    assert set(rows) == set(rec), (sorted(rows), sorted(rec))
    for k, (msims, us) in rows.items():
        assert abs(msims - rec[k]["value"] / 1e6) < 0.05, k
        assert abs(us - rec[k]["avg_launch_us"]) < 0.006, k


def test_source_map_is_the_sources():
    """DESIGN §3's "Source map" against mazero_amd/csrc/: every .inc part is included by exactly one
    `#include "..."` line of a .hip or .inc file of the folder, the table lists exactly the folder's
    .hip, .inc and .h files, and every kernel a row names is defined in that row's file (with its
    body: a declaration does not count)."""
    csrc = os.path.join(ROOT, "mazero_amd", "csrc")
    files = sorted(n for n in os.listdir(csrc) if n.endswith((".hip", ".inc", ".h")))
    src = {}
    for n in files:
        with open(os.path.join(csrc, n)) as f:
            src[n] = f.read()
    includes = [m for n in files if n.endswith((".hip", ".inc"))
                for m in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', src[n], flags=re.M)]
    for n in files:
        if n.endswith(".inc"):
            assert includes.count(n) == 1, f"{n} is included {includes.count(n)} times"
    text = _read("DESIGN.md")
    sec = text[text.index("### Source map"):text.index("### Build switches")]
    rows = re.findall(r"^\| `([A-Za-z0-9_.]+)` \|[^|]*\|([^|]*)\|$", sec, flags=re.M)
    assert sorted(r[0] for r in rows) == files, (sorted(r[0] for r in rows), files)
    named = 0
    for name, cell in rows:
        for k in re.findall(r"`(k_\w+)`", cell):
            named += 1
            assert re.search(r"__global__[^;{()]*(\([^()]*\)[^;{()]*)*\bvoid\s+" + k + r"\s*\([^;{]*\{", src[name]), (name, k)
    assert named, "the Source map names no kernel"
    # and the other way round: a kernel no row names has no documented home
    for n in files:
        cell = dict(rows)[n]
        for k in re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src[n]):
            assert f"`{k}`" in cell, (n, k)
