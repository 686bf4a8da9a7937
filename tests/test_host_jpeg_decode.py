"""No GPU: the definition of the device Motion-JPEG decoder (evaluate.py --device_decode 1).  The restatement in
jpeg_decode_refs.py against PIL byte for byte on every stream of jpeg_decode_cases.py; evaluate.jpeg_parse on those streams and on
files it must refuse; the per-lane entropy step the kernels run (csrc/jpeg_decode_core.h), compiled into a stand-alone host program
with the address / undefined-behaviour sanitizers, against the restatement and over damaged streams; the flag."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_decode_cases as C

import egne_amd  # noqa: F401
from egne_amd import evaluate as E

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = list(C.cases())


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pil(name):
    """The contract: the current host path, np.asarray(Image.open(...).convert('L')) -- and PIL's RGB for colour files."""
    j = C.cases()[name]
    coef, L, rgb = C.reference(name)
    im = Image.open(io.BytesIO(j))
    assert np.array_equal(np.asarray(im.convert("L")), L)
    assert (im.mode == "L" and rgb is None) or np.array_equal(np.asarray(im), rgb)
    if rgb is not None and not name.startswith("video_"):
        assert (rgb[..., 0] != rgb[..., 1]).any()              # the colour path is exercised (the video's chroma is neutral)


def test_restart_streams_have_their_markers():
    for name, r in (("restart_1", 1), ("restart_3", 3), ("restart_8", 8), ("restart_pil_3", 3), ("restart_pil_grey_2", 2)):
        info = E.jpeg_parse(C.cases()[name])
        assert info["restart"] == r
        scan = C.cases()[name][info["scan_off"]: info["scan_off"] + info["scan_len"]]
        nmcu = -(-info["H"] // (16 if info["sampling"] == E.JPEG_420 else 8)) * -(-info["W"] // (16 if info["sampling"] == E.JPEG_420 else 8))
        assert sum(scan.count(bytes((0xFF, 0xD0 + m))) for m in range(8)) == -(-nmcu // r) - 1 > 0


@pytest.mark.parametrize("name", NAMES)
def test_parse_accepts(name):
    j = C.cases()[name]
    info = E.jpeg_parse(j)
    assert info is not None
    im = Image.open(io.BytesIO(j))
    assert (info["W"], info["H"]) == im.size
    want = {"grey": E.JPEG_GREY, "444_": E.JPEG_444, "422_": E.JPEG_422}
    assert info["sampling"] == next((v for k, v in want.items() if name.startswith(k)), E.JPEG_GREY if im.mode == "L" else E.JPEG_420)
    assert j[info["scan_off"] + info["scan_len"]: info["scan_off"] + info["scan_len"] + 2] == b"\xff\xd9"
    assert j[info["scan_off"] - 3: info["scan_off"]] == b"\x00\x3f\x00"           # right behind SOS
    assert info["record"].shape == (E.JPEG_DESC_BYTES,) and len(info["components"]) == (1 if im.mode == "L" else 3)
    assert all(len(q) == 64 for q in info["qt"].values())
    used = {("dc", c[3]) for c in info["components"]} | {("ac", c[4]) for c in info["components"]}
    for kind, t in used:
        counts, symbols = info["huff"][t if kind == "dc" else 2 + t]
        assert len(counts) == 16 and sum(counts) == len(symbols)
    if name == "no_dht_29x37":
        assert b"\xff\xc4" not in j[:info["scan_off"]]
        assert [info["huff"][t] for t in (0, 2, 1, 3)] == [(bytes(c), bytes(s)) for c, s in E._JPEG_HUFF]
    if name == "optimize_29x37":
        assert info["huff"][2] != (bytes(E._JPEG_HUFF[1][0]), bytes(E._JPEG_HUFF[1][1]))


def _edit(j, marker, fn):
    """The file with the body of its first `marker` segment replaced by fn(body) (same length)."""
    p = 2
    while True:
        m, n = j[p + 1], int.from_bytes(j[p + 2: p + 4], "big")
        if m == marker:
            body = fn(bytearray(j[p + 4: p + 2 + n]))
            assert len(body) == n - 2
            return j[:p + 4] + bytes(body) + j[p + 2 + n:]
        assert m != 0xDA
        p += 2 + n


def test_parse_refuses_what_the_device_does_not_take():
    img = C.colour_image(29, 37, 5)
    base = C._pil(img, quality=60, subsampling=2)
    assert E.jpeg_parse(base) is not None
    assert E.jpeg_parse(C._pil(img, quality=60, progressive=True)) is None
    assert E.jpeg_parse(base.replace(b"\xff\xc0", b"\xff\xc2", 1)) is None                     # SOF0 -> SOF2 in the header

    def twelve(b):
        b[0] = 12
        return b
    assert E.jpeg_parse(_edit(base, 0xC0, twelve)) is None

    def four_one_one(b):
        b[7] = 0x41
        return b
    assert E.jpeg_parse(_edit(base, 0xC0, four_one_one)) is None
    info = E.jpeg_parse(base)
    sos = base[info["scan_off"] - 14: info["scan_off"]]
    assert sos[:2] == b"\xff\xda"
    scan_end = info["scan_off"] + info["scan_len"]
    two_scans = base[:scan_end] + sos + base[info["scan_off"]:]
    assert E.jpeg_parse(two_scans) is None

    def sixteen_bit(b):
        b[0] |= 0x10
        return b
    assert E.jpeg_parse(_edit(base, 0xDB, sixteen_bit)) is None
    assert E.jpeg_parse(base[:scan_end - 5] + b"\xff\xff" + base[scan_end - 5:]) is None       # fill bytes inside the scan
    assert E.jpeg_parse(C._pil(C.colour_image(8, 4), quality=90, subsampling=2)) is None       # chroma plane of two columns
    assert E.jpeg_parse(C._pil(C.colour_image(8, 5), quality=90, subsampling=2)) is not None
    assert E.jpeg_parse(b"") is None and E.jpeg_parse(base[:100]) is None and E.jpeg_parse(b"\xff\xd8\xff\xd9") is None
    assert E.jpeg_parse(base) is not None                                                       # (the header cache did not go stale)


def test_parse_refuses_three_components_that_are_not_ycbcr():
    """Without a JFIF segment libjpeg (and PIL) take component identifiers 'R', 'G', 'B' and an Adobe segment with transform 0 for
    RGB data and skip the colour conversion: such files differ from the device's YCbCr decode, so they go to the host."""
    j = C.cases()["444_24x40"]
    assert j[2:4] == b"\xff\xe0"
    plain = j[:2] + j[4 + int.from_bytes(j[4:6], "big"):]                 # the JFIF segment cut out: still YCbCr (identifiers 1, 2, 3)
    want = np.asarray(Image.open(io.BytesIO(j)).convert("L"))
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(plain)).convert("L")), want) and E.jpeg_parse(plain) is not None
    b, sof, sos = bytearray(plain), plain.index(b"\xff\xc0"), plain.index(b"\xff\xda")
    for k, c in enumerate(b"RGB"):
        b[sof + 10 + 3 * k] = b[sos + 5 + 2 * k] = c
    adobe = lambda t: plain[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t]) + plain[2:]      # noqa: E731
    for other in (bytes(b), adobe(0)):
        assert not np.array_equal(np.asarray(Image.open(io.BytesIO(other)).convert("L")), want)
        assert E.jpeg_parse(other) is None
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(adobe(1))).convert("L")), want) and E.jpeg_parse(adobe(1)) is not None


def test_narrow_chroma_is_why_those_files_are_refused():
    """libjpeg replicates a subsampled chroma plane of one or two columns instead of interpolating it: the restatement's (and the
    kernel's) formula differs from PIL there, so jpeg_parse must not take such files."""
    import jpeg_decode_refs as D
    differs = False
    for seed in range(4):
        j = C._pil(C.colour_image(16, 4, seed), quality=95, subsampling=2)
        differs |= not np.array_equal(D.decode(j)[0], np.asarray(Image.open(io.BytesIO(j)).convert("L")))
    assert differs


def test_chunks_are_the_frames(tmp_path):
    """mjpeg_chunks yields the very files mjpeg_frames decodes, in its order."""
    w = E.MJPEGWriter(str(tmp_path / "a.avi"), 30, (56, 40))
    imgs = [np.ascontiguousarray(C.colour_image(40, 56, s)[..., ::-1]) for s in range(3)]
    for im in imgs:
        w.write(im)
    w.release()
    chunks = list(E.mjpeg_chunks(str(tmp_path / "a.avi")))
    frames = list(E.mjpeg_frames(str(tmp_path / "a.avi")))
    assert len(chunks) == len(frames) == 3
    for c, f in zip(chunks, frames):
        assert c[:2] == b"\xff\xd8" and c[-2:] == b"\xff\xd9"
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(c)).convert("L")), f)
        assert np.array_equal(E._decode_host(c), f)
    assert E._decode_host(b"\xff\xd8\xff\xd9") is None


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: the entropy step's bounds rules are proven by this program")
    d = tmp_path_factory.mktemp("jpeg_decode_host")
    exe = str(d / "jpeg_decode_host")
    # the sanitizer runtimes are linked statically (clang's default; g++ needs the two switches): the program then does not depend
    # on the order in which shared objects are loaded, whatever the environment it inherits
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                          ["-o", exe, os.path.join(HERE, "jpeg_decode_host.cpp")])
    blob = [np.int32(len(NAMES)).tobytes()]
    for name in NAMES:
        j = C.cases()[name]
        info = E.jpeg_parse(j)
        scan = j[info["scan_off"]: info["scan_off"] + info["scan_len"]]
        scan += b"\0" * (-len(scan) % 4)
        rec = info["record"].copy()
        rec[:32].view(np.int32)[:2] = (0, info["scan_len"])
        blob += [np.array([info["H"], info["W"], info["sampling"], len(scan)], np.int32).tobytes(), rec.tobytes(), scan]
    with open(str(d / "cases.bin"), "wb") as f:
        f.write(b"".join(blob))
    p = subprocess.run([exe, str(d / "cases.bin"), str(d / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    print(p.stdout.decode())
    print(p.stderr.decode())
    return p, open(str(d / "out.bin"), "rb").read()


def test_host_program_ends_clean(host_program):
    """Every case, every case cut off at half its scan and with 32 single-bit flips, at sub_bits 128 and 1024 and in windows of 5
    and 256 lanes: no sanitizer report, mode 1 equal to mode 0 everywhere (a flag or a decode)."""
    p, _ = host_program
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert b"ERROR" not in p.stderr and b"runtime error" not in p.stderr
    last = p.stdout.decode().strip().splitlines()[-1]
    assert last.startswith("damaged:") and int(last.split()[1]) == len(NAMES) * 33 * 2
    assert int(last.split()[3]) > len(NAMES)                     # damage is noticed: at least the cut streams, and flips beyond them
    assert int(last.split()[-2]) > 1                             # more than one synchronisation round somewhere at sub_bits 128


@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_host_program_equals_the_restatement(host_program, k):
    p, out = host_program
    assert p.returncode == 0
    at = 0
    for i in range(k + 1):
        flag, blocks = np.frombuffer(out, np.int32, 2, at)
        coef = np.frombuffer(out, np.int16, blocks * 64, at + 8).reshape(blocks, 64)
        at += 8 + blocks * 128
    want = C.reference(NAMES[k])[0]
    assert flag == 0 and coef.shape == want.shape
    assert np.array_equal(coef, want)


def test_flag():
    assert E.parse_args([]).device_decode == 0
    a = E.parse_args(["--device_io", "1", "--device_decode", "1"])
    assert a.device_decode == 1 and a.device_io == 1 and a.device_jpeg == 0
    with pytest.raises(SystemExit):
        E.parse_args(["--device_decode", "1"])
    with pytest.raises(SystemExit):
        E.parse_args(["--device_io", "0", "--device_decode", "1"])


def test_decode_jpeg_device_checks_on_the_host():
    c = C.cases()
    with pytest.raises(ValueError, match="geometry"):
        E.decode_jpeg_device([c["restart_1"], c["420_16x16"]])
    with pytest.raises(ValueError, match="sampling"):
        E.decode_jpeg_device([c["444_24x40"], c["422_24x40"]])
    with pytest.raises(ValueError, match="jpeg_parse"):
        E.decode_jpeg_device([c["restart_1"], b"\xff\xd8\xff\xd9"])
    with pytest.raises(ValueError):
        E.decode_jpeg_device([])
