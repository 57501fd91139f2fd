"""README's table of environment knobs against the code: every AMMC_* variable the package or the library reads is listed
there, and every variable listed there is still read somewhere (a retired name cannot come back unnoticed, a new one
cannot stay undocumented)."""
import glob
import os
import re

from conftest import ROOT

PKG = os.path.join(ROOT, "ammcnet_aaai2021_amd")
NAME = r"AMMC_[A-Z0-9_]+"


def _text(*patterns):
    files = [f for p in patterns for f in sorted(glob.glob(os.path.join(ROOT, p), recursive=True)) if os.path.isfile(f)]
    return "\n".join(open(f, errors="replace").read() for f in files)


def _knob_section():
    readme = open(os.path.join(ROOT, "README.md")).read()
    start = readme.index("Environment knobs")
    rows = re.match(r"[^\n]*\n\n((?:\|[^\n]*\n)+)", readme[start:]).group(1)
    return rows, [r.split("|")[1] for r in rows.splitlines()[2:]]


def test_every_variable_the_package_reads_is_in_the_table():
    read = set(re.findall(r'getenv\("(%s)"\)' % NAME, _text("ammcnet_aaai2021_amd/csrc/*.hip", "ammcnet_aaai2021_amd/csrc/*.h")))
    read |= set(re.findall(r'environ(?:\.get\(|\[)"(%s)"' % NAME, _text("ammcnet_aaai2021_amd/*.py")))
    assert len(read) > 20                                                      # (the patterns still find the reads)
    rows, _ = _knob_section()
    documented = set(re.findall(r"`(%s)[`=]" % NAME, rows))
    assert read <= documented, sorted(read - documented)


def test_every_variable_of_the_table_is_read_somewhere():
    _, first = _knob_section()
    listed = {n for cell in first for n in re.findall(NAME, cell)}
    assert len(listed) > 20
    code = _text("ammcnet_aaai2021_amd/*.py", "ammcnet_aaai2021_amd/csrc/*", "bench.py", "tests/**/*.py", "tools/**/*")
    read = set(re.findall(r'getenv\("(%s)"' % NAME, code)) | set(re.findall(r'environ(?:\.get\(|\[)"(%s)"' % NAME, code))
    read |= set(re.findall(r"#\s*if(?:n?def\s+|.*defined\s*\(?\s*)(%s)" % NAME, _text("ammcnet_aaai2021_amd/csrc/*")))       # -D macros
    assert listed <= read, sorted(listed - read)
