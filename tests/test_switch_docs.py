"""CPU: README "Switches" and the environment variables the package reads name the same things (plain text, no import of the
package): a variable the code reads is documented, and a training / loss switch the README offers is still read."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_READ = re.compile(r"""os\.environ(?:\.get\(|\[)\s*["'](PF_[A-Z0-9_]+)["']""")
REMOVED = "removed after commit"          # the one sentence (line) that names the switches that are gone


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _env_reads():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "puflow_amd", "*.py")):
        names.update(ENV_READ.findall(_read(path)))
    return names


def test_every_variable_the_package_reads_is_in_the_readme():
    reads = _env_reads()
    assert "PF_TRAIN_FUSED" in reads and "PF_LIB_PATH" in reads, "the pattern no longer finds the reads"
    readme = set(re.findall(r"PF_[A-Z0-9_]+", _read(os.path.join(ROOT, "README.md"))))
    assert not sorted(reads - readme), f"read through os.environ but not in README.md: {sorted(reads - readme)}"


def test_every_training_switch_in_the_readme_is_still_read():
    reads = _env_reads()
    lines = _read(os.path.join(ROOT, "README.md")).splitlines()
    assert sum(REMOVED in ln and "PF_TRAIN_" in ln for ln in lines) == 1, "one sentence names the removed switches"
    offered = set()
    for ln in lines:
        if REMOVED not in ln:
            offered.update(re.findall(r"PF_(?:TRAIN|LOSS)_[A-Z0-9_]+", ln))
    assert "PF_TRAIN_FUSED" in offered
    assert not sorted(offered - reads), f"in README.md but read nowhere in puflow_amd/: {sorted(offered - reads)}"
