"""The host's reader of state images and deltas (vigor_amd/csrc/vp_state_img.h:
what vp_state_load and vp_state_delta_apply check before anything is uploaded)
built alone with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/state_reader_main.cc) and run as a child
process over images and deltas packed on the CPU: intact ones pass, the
header-level mutations are refused with the text the library gave on the GPU
(tests/golden/state_messages.json), every truncation is refused, and no run
ends with a sanitizer's report. CPU only."""
import os
import shutil
import subprocess

import pytest

import deltacases as DC
import deltaref as DR
import statecases as SC
import stateref as SR

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -22
MARK = (77, 3)


@pytest.fixture(scope="module")
def reader(tmp_path_factory):
    cxx = next((c for c in ("g++", "clang++", "c++") if shutil.which(c)), None)
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("reader") / "state_reader_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(HERE, "state_reader_main.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tmp = tmp_path_factory.mktemp("blobs")

    def run(blob, fmt, kind, *flags):
        path = str(tmp / "blob")
        with open(path, "wb") as f:
            f.write(blob)
        caps = [str(SC.CAP)] + ([str(SC.LB_BCAP)] if kind == "lb" else [])
        r = subprocess.run([exe, path, fmt, kind] + caps + list(flags), capture_output=True,
                           text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr  # (a report ends the run with 1)
        lines = [ln.split(" ", 1) for ln in r.stdout.splitlines()]
        return [[int(rc), text] for rc, text in lines]
    return run


def _delta(kind):
    s0, s1, touched = DC.victim(kind, cap=SC.CAP, bcap=SC.LB_BCAP)
    return s0, DR.diff(s0, s1, touched, base=MARK, mark=(MARK[0] + 40, MARK[1]))


@pytest.mark.parametrize("kind", ["nat", "lb"])
def test_images(reader, kind):
    img = SR.pack(SC.small_state(kind))
    assert reader(img, "image", kind) == [[0, ""]]
    muts, want = SC.mutations(kind, img), SC.recorded()["image_small"][kind]
    names = [m for m in SC.HEADER_LEVEL if m in muts]
    assert sorted(names) == sorted(want) and len(names) >= 9
    for name in names:
        assert reader(muts[name], "image", kind) == [want[name]], name


@pytest.mark.parametrize("kind", ["fw", "lb"])
def test_deltas(reader, kind):
    s0, good = _delta(kind)
    assert reader(DR.pack(good), "delta", kind) == [[0, ""]]
    muts, want = DC.mutations(s0, good), SC.recorded()["delta"][kind]
    names = [m for m in DC.HEADER_LEVEL if m in muts]
    assert len(names) >= 12
    for name in names:
        assert reader(muts[name], "delta", kind) == [want[name]], name


@pytest.mark.parametrize("fmt,kind", [("image", "nat"), ("delta", "lb")])
def test_every_truncation_is_refused(reader, fmt, kind):
    blob = SR.pack(SC.small_state(kind)) if fmt == "image" else DR.pack(_delta(kind)[1])
    got = reader(blob, fmt, kind, "--truncations")
    assert len(got) == len(blob) + 1 and got[-1] == [0, ""]
    prefix = "state load: " if fmt == "image" else "state delta apply: "
    for n, (rc, text) in enumerate(got[:-1]):
        assert rc == EINVAL and text.startswith(prefix), (n, rc, text)
