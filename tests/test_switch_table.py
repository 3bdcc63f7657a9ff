"""The environment switches have one home.  A text check of the sources against profiles/SWITCHES.md (builds nothing):
the compressor's host sources call getenv only in the switch table (switches.h), for the process-wide measuring aids
(host_support.h), in the read library (archive_read.h) and in the CLI (main.cpp); every name they read is documented; every
AGC_AMD_* behaviour switch the document lists is read somewhere under agc_amd/."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "agc_amd", "csrc", "host")
MAY_READ = {"switches.h", "host_support.h", "archive_read.h", "main.cpp"}
GETENV = re.compile(r'getenv\s*\(\s*("([A-Za-z0-9_]+)")?')


def _text(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _host_reads():
    """{file name: [names read]}; a getenv whose argument is not a string literal counts as the name None"""
    reads = {}
    for path in sorted(glob.glob(os.path.join(HOST, "*.cpp")) + glob.glob(os.path.join(HOST, "*.h"))):
        names = [m.group(2) for m in GETENV.finditer(_text(path))]
        if names:
            reads[os.path.basename(path)] = names
    return reads


def _switch_rows():
    """the backquoted AGC_AMD_* names in the first column of the behaviour-switch table"""
    names = []
    for line in _text(os.path.join(ROOT, "profiles", "SWITCHES.md")).splitlines():
        if not line.startswith("| `"):
            continue
        first = re.split(r"(?<!\\)\|", line)[1]
        names += re.findall(r"`(AGC_AMD_[A-Z0-9_]+)", first)
    return names


def test_getenv_lives_in_the_switch_table_only():
    reads = _host_reads()
    assert "switches.h" in reads and len(reads["switches.h"]) >= 25, "the table was not found"
    outside = {f: n for f, n in reads.items() if f not in MAY_READ}
    assert not outside, "getenv outside the switch table: %r" % outside
    computed = {f: n for f, n in reads.items() if None in n}
    assert not computed, "getenv of a name that is not a string literal: %r" % sorted(computed)


def test_every_switch_read_is_documented():
    doc = _text(os.path.join(ROOT, "profiles", "SWITCHES.md"))
    missing = sorted({n for names in _host_reads().values() for n in names if n and not re.search(r"\b%s\b" % n, doc)})
    assert not missing, "read by the host sources, not in profiles/SWITCHES.md: %r" % missing


def test_every_documented_switch_is_read():
    rows = _switch_rows()
    assert len(rows) >= 25, rows  # (the table was found and parsed)
    src = ""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "agc_amd")):
        if os.path.basename(dirpath) in ("__pycache__", "_build"):
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip", ".c")):
                src += _text(os.path.join(dirpath, f))
    unread = sorted(n for n in set(rows) if not re.search(r'(getenv\s*\(|environ\.get\s*\(|environ\s*\[)\s*"%s"' % n, src))
    assert not unread, "documented in profiles/SWITCHES.md, read nowhere under agc_amd/: %r" % unread
