"""The switches of a context are listed once in the code (kOptions, unified_cvo_amd/csrc/cvo_options.h) and once for the
reader (the switch table of INTEGRATION.md): both name the same set.  Reads source text, builds nothing."""
import os
import re

import cases


def _table_names():
    """The names of kOptions: the first string literal of every entry of the table."""
    text = open(os.path.join(cases.ROOT, "unified_cvo_amd", "csrc", "cvo_options.h")).read()
    body = re.search(r"constexpr OptionSpec kOptions\[\] = \{(.*?)\n\};", text, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return re.findall(r"^\s*(?:opt_\w+\(|\{)\"([A-Z0-9_]+)\"", body, flags=re.M)


def _documented_names():
    """CVO_<NAME> in the first column of the table under "Environment switches" in INTEGRATION.md."""
    text = open(os.path.join(cases.ROOT, "INTEGRATION.md")).read()
    section = text.split("## Environment switches of `libcvo_hip.so`", 1)[1].split("\n## ", 1)[0]
    names = []
    for line in section.splitlines():
        if line.startswith("| `CVO_"):
            names += re.findall(r"`CVO_([A-Z0-9_]+)", line.split("|")[1])
    return names


def test_every_switch_of_the_code_is_documented_and_none_else():
    table, documented = _table_names(), _documented_names()
    assert len(table) > 20 and len(set(table)) == len(table), table
    assert len(set(documented)) == len(documented), documented
    assert set(documented) - {"QUIET"} == set(table)  # (CVO_QUIET is read per process, where the advice is printed)


def test_no_switch_is_looked_up_by_name_outside_the_table():
    csrc = os.path.join(cases.ROOT, "unified_cvo_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, f)).read()
        assert "ctx_opt" not in text, f
        if f != "cvo_ctx.hip":  # (cvo_ctx_create: the environment, through the table; the hardware-queue advice)
            assert "getenv" not in text, f
