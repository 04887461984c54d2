"""The plans and scratch layouts of the post-processing on the CPU: tools/post_plan.cpp
(csrc/post_plan.cpp alone, no device).

golden/post_plans.txt holds "case | plan | layout" lines under the default switches, and per
switch setting the fields of each line that differ from them (_sections rebuilds the lines): the rows of
_post_edges.BODY_CASES, the known geometries of test_post_plan_api.py at 1, 2, 6 and 32 frames for
both body kinds, and the hand crops of _post_edges and 92, 184, 192, 193, 368, 736.  The plan fields
are the ones the library before post_plan.cpp returned for the same case and setting; the
layouts were held to that library's pointer carving on the GPU (profiles/postplan/README.md).
The tool, which reads the switches from its environment as a post does, must print the same lines.
"""
import functools
import os
import re
import shutil
import subprocess

import pytest

import _post_edges as pe

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "isl-signlanguage-translation_amd", "csrc")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_plans.txt")

BODY_REGIONS = ("heat", "mid", "mask", "pairs", "used", "live", "bandmax", "amb", "bm1", "live_mid", "need")
HAND_REGIONS = ("avg", "mid", "mask", "parent", "vals", "stats", "chunks", "bsum", "amb")


def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("amdclang++")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no ROCm host compiler")
    exe = str(tmp_path_factory.mktemp("post_plan") / "post_plan")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + os.path.join(REPO, "include"),
                    "-I" + CSRC, os.path.join(REPO, "tools", "post_plan.cpp"), os.path.join(CSRC, "post_plan.cpp"),
                    "-o", exe], check=True, timeout=300)
    return exe


ENV_ORDER = ("FUSED_BLUR", "FUSED_WIDE", "BLUR_LIST", "BLUR_BANDS", "RESIZE_SKIP", "RESIZE_V4", "BLUR_EXACT", "LIMB_LDS",
             "ASM_REG")          # the entries of the body plan's env= (tools/post_plan.cpp)


def _under(line, setting, diffs):
    """The [] line of a case as it stands under `setting`: the fields of `diffs` ("k=v ...")
    replaced, and for a body case the switch's own entry of env= set to its value's first digit."""
    new = dict(kv.split("=") for kv in diffs.split())
    name, value = setting.split("=")
    parts = []
    for part in line.split(" | "):
        toks = part.split(" ")
        for i, t in enumerate(toks):
            k, eq, v = t.partition("=")
            if eq and k in new:
                toks[i] = k + "=" + new.pop(k)
            elif eq and k == "env" and name[len("ISLPOSE_"):] in ENV_ORDER:
                e = v.split(",")
                e[ENV_ORDER.index(name[len("ISLPOSE_"):])] = value[0]
                toks[i] = "env=" + ",".join(e)
        parts.append(" ".join(toks))
    assert not new, (line, diffs)
    return " | ".join(parts)


@functools.lru_cache(maxsize=None)
def _sections():
    """((switch setting "NAME=value" or "", (the tool's lines of every case under it)), ...) of the
    golden file: section [] as written, every other section rebuilt from its differences."""
    raw = []
    with open(GOLDEN) as f:
        for ln in f.read().splitlines():
            if not ln.strip() or ln.startswith("#"):
                continue
            m = re.fullmatch(r"\[(.*)\]", ln)
            if m:
                raw.append((m.group(1), []))
            else:
                raw[-1][1].append(ln)
    assert raw[0][0] == ""
    base = raw[0][1]
    cases = [ln.split(" | ")[0] for ln in base]
    out = [("", tuple(base))]
    for setting, lines in raw[1:]:
        diffs = dict(ln.split(" | ") for ln in lines)
        # (a case that stands twice in [] stands twice here, with the same differences)
        assert set(diffs) <= set(cases), setting
        assert all(diffs[c] == d for c, d in (ln.split(" | ") for ln in lines)), setting
        out.append((setting, tuple(_under(b, setting, diffs.get(c, "")) for b, c in zip(base, cases))))
    return tuple(out)


def _switch_table(tool):
    """[(name, default, values)] of post_plan --switches."""
    return [ln.split() for ln in subprocess.run([tool, "--switches"], check=True, timeout=60, capture_output=True,
                                                 text=True).stdout.splitlines()]


def _parse(line):
    case, plan, lay = [p.strip() for p in line.split("|")]
    return case.split(), dict(kv.split("=") for kv in plan.split()), dict(kv.split("=") for kv in lay.split())


def test_tool_prints_the_golden_lines(tool, tmp_path):
    table = _switch_table(tool)
    env = {k: v for k, v in os.environ.items() if k not in {t[0] for t in table}}
    sections = _sections()
    assert sum(len(lines) for _, lines in sections) >= 1000
    for setting, want in sections:
        e = dict(env)
        if setting:
            k, v = setting.split("=")
            e[k] = v
        got = subprocess.run([tool, _cases_file(tmp_path, want)], check=True, timeout=120, capture_output=True,
                             text=True, env=e).stdout.splitlines()
        bad = [(w, g) for w, g in zip(want, got) if w != g]
        assert not bad, "[%s] %d of %d lines differ, the first:\ngolden %s\ntool   %s" % (setting, len(bad), len(want), *bad[0])
        assert len(got) == len(want)


def _cases_file(tmp_path, lines):
    p = tmp_path / "cases.txt"
    p.write_text("\n".join(ln.split("|")[0] for ln in lines) + "\n")
    return str(p)


def test_golden_covers_every_switch_and_case(tool):
    """Every switch of the table singly at each documented value, the same cases in every section;
    the cases the header names are there."""
    sections = _sections()
    settings = [s for s, _ in sections]
    assert settings[0] == "" and len(set(settings)) == len(settings)
    for name, default, values in _switch_table(tool):
        vals = values.split("..") if ".." in values else list(values)
        for v in vals:
            assert "%s=%s" % (name, v) in settings, (name, v)
    cases = [ln.split("|")[0] for ln in sections[0][1]]
    for _, lines in sections[1:]:
        assert [ln.split("|")[0] for ln in lines] == cases
    parsed = [c.split() for c in cases]
    body = {(c[1], int(c[2]), int(c[3]), int(c[4]), int(c[5])) for c in parsed if c[0] == "body"}
    hand = {(int(c[1]), int(c[2]), int(c[3])) for c in parsed if c[0] == "hand"}
    for kind, H, W, scales, _, _ in pe.BODY_CASES.values():
        assert (kind, 2, H, W, len(scales)) in body
    for H, W, ns in ((184, 328, 1), (368, 656, 1), (1080, 1920, 1), (240, 320, 1), (240, 328, 2)):
        for kind in ("body25", "coco"):
            for n in (1, 2, 6, 32):
                assert (kind, n, H, W, ns) in body
    for s in pe.HAND_SQUARE + (92, 184, 192, 193, 368, 736):
        assert (1, s, s) in hand
    assert (1,) + pe.HAND_RECT in hand


def test_layouts_are_well_formed():
    """Every line: the regions in the documented order, each at a multiple of 256 bytes, none
    overlapping the next, total the end of the last; a region the plan does not use has no bytes."""
    n_lines = 0
    for _, lines in _sections():
        for ln in lines:
            case, plan, lay = _parse(ln)
            names = BODY_REGIONS if case[0] == "body" else HAND_REGIONS
            assert list(lay)[:len(names)] == list(names) and list(lay)[len(names)] == "total", ln
            reg = [tuple(int(v) for v in lay[k].split("+")) for k in names]
            total = int(lay["total"])
            assert reg[0][0] == 0
            for (off, size), (nxt, _) in zip(reg, reg[1:] + [(total, 0)]):
                assert off % 256 == 0 and off <= nxt and off + size <= nxt and nxt - (off + size) < 256, ln
            assert total % 256 == 0
            size = dict(zip(names, (r[1] for r in reg)))
            if case[0] == "body":
                fused, multi, skip2 = int(plan["fused"]), int(plan["multi"]), int(plan["skip2"])
                assert (size["heat"] == 0) == bool(fused), ln
                assert (size["mid"] == 0) == (not any(int(v) for v in plan["scale_two_stage"].split(","))), ln
                for k in ("bm1", "live_mid", "need"):
                    assert (size[k] != 0) == bool(skip2), ln
                # the band maxima and the live list: wherever a plan uses them, and never for a fused
                # or multi-scale post's bands (they are sized by the switch: post_plan.cpp)
                if plan["final"].split(",")[0].split(":")[4] == "1" or int(plan["blur_bandmax"]):
                    assert size["bandmax"], ln
                if fused or multi:
                    assert not size["bandmax"], ln
                if plan["blur"] in ("FUSED_LIVE", "BAND_LIVE"):
                    assert size["live"], ln
                if multi:
                    assert not size["live"], ln
                assert size["live"] in (0, size["amb"]) and size["amb"] == 4 * (int(lay["tiles"]) + 1), ln
                assert all(size[k] for k in ("mask", "pairs", "used", "amb")), ln
            else:
                assert (size["mid"] == 0) == (not any(int(v) for v in plan["two_stage"].split(","))), ln
                assert all(size[k] for k in HAND_REGIONS if k != "mid"), ln
            n_lines += 1
    assert n_lines >= 1000


def test_hand_layout_of_one_crop_is_the_lane_size(tool, tmp_path):
    """isl_hand_post_crops_ex sizes a lane by hand_post_layout(...).total of one crop, the call
    hand_post_launch carves by: post.hip has one function for both, and the n = 1 line of a crop
    gives the same total wherever it stands in a file of other cases."""
    src = open(os.path.join(CSRC, "post.hip")).read()
    assert src.count("hand_post_layout(") == 1 and "hand_post_bytes" not in src
    assert len(re.findall(r"\bhand_layout\(1, crop_w\[i\], crop_w\[i\]", src)) == 1
    ones = [ln for ln in _sections()[0][1] if ln.startswith("hand 1 ")]
    assert len(ones) >= 15
    mixed = [ln for pair in zip(ones, reversed(ones)) for ln in pair]
    got = subprocess.run([tool, _cases_file(tmp_path, mixed)], check=True, timeout=60, capture_output=True,
                         text=True).stdout.splitlines()
    assert got == mixed


def test_switches_are_read_in_one_place():
    """getenv: in post_plan.cpp only inside post_switches(), nowhere in post.hip; neither
    post_plan file includes a HIP header."""
    with open(os.path.join(CSRC, "post.hip")) as f:
        assert "getenv" not in f.read()
    with open(os.path.join(CSRC, "post_plan.cpp")) as f:
        src = f.read()
    body = re.search(r"\nPostSwitches post_switches\(\) \{\n(.*?)\n\}\n", src, re.S)
    assert body and body.group(1).count("getenv") == 1
    assert src.count("getenv(") == 1
    for name in ("post_plan.cpp", "post_plan.h"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        assert "hip" not in " ".join(re.findall(r"#include\s+\S+", text)).lower()
        assert "__global__" not in text
