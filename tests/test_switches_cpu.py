"""Environment switches: each is read one way, every per-call read is in the step-program key, and §10 names exactly
the switches the package reads.

A step program replays a recorded launch list, so a switch that the library reads on every call and that changes that list must be
part of the step-program key (wgan._KEY_ENV); every other dispatch switch in csrc is read once into a function-local static."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "blurred-gan_amd")
CSRC = os.path.join(PKG, "csrc")
NAME = r"BG(?:AN)?_[A-Z0-9_]*[A-Z0-9]"


def _csrc_reads():
    """(read once, read per call): the getenv names of csrc, by whether the read sits on a `static const` line."""
    once, per_call = set(), set()
    for f in sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))):
        for line in open(os.path.join(CSRC, f)):
            code = line.split("//")[0]
            names = re.findall(r'getenv\("(\w+)"\)', code)
            assert len(names) == code.count("getenv("), f"{f}: getenv without a literal name: {line.strip()}"
            (once if re.search(r"\bstatic const\b", code) else per_call).update(names)
    return once, per_call


def _python_reads():
    names = set()
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py"):
                names.update(re.findall(rf"[\"']({NAME})[\"']", open(os.path.join(dirpath, f)).read()))
    return names


def _design_rows():
    """(names, read column) of every table row of DESIGN.md §10; build-time -D names are left out."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 10. Environment switches"):]
    nxt = sec.find("\n## ", 1)
    rows = []
    for line in (sec if nxt < 0 else sec[:nxt]).splitlines():
        if not line.startswith("| `"):
            continue
        cells = [c.strip() for c in re.split(r"(?<!\\)\|", line.strip().strip("|"))]
        names = {m.group(2) for m in re.finditer(rf"(-D)?\b({NAME})\b", cells[0]) if not m.group(1)}
        rows.append((names, cells[1] if len(cells) > 2 else None))
    return rows


def test_each_csrc_switch_is_read_one_way():
    once, per_call = _csrc_reads()
    assert once and per_call
    assert not once & per_call, sorted(once & per_call)


def test_per_call_csrc_switches_are_the_step_key():
    from blurred_gan_amd import wgan
    _, per_call = _csrc_reads()
    assert per_call == {n for n in wgan._KEY_ENV if n.startswith("BG_")}
    assert len(set(wgan._KEY_ENV)) == len(wgan._KEY_ENV)


def test_design_names_exactly_the_switches_read():
    once, per_call = _csrc_reads()
    read = once | per_call | _python_reads()
    documented = set().union(*(names for names, _ in _design_rows()))
    assert read - documented == set(), "read but not in DESIGN.md §10"
    assert documented - read == set(), "in DESIGN.md §10 but read nowhere"


def test_design_marks_how_each_switch_is_read():
    from blurred_gan_amd import wgan
    once, _ = _csrc_reads()
    marked = {}
    for names, how in _design_rows():
        for n in names:
            marked.setdefault(n, set()).add(how)
    for n in wgan._KEY_ENV:
        assert marked[n] == {"per call (step key)"}, (n, marked[n])
    for n in once:
        assert marked[n] == {"once"}, (n, marked[n])
