"""CPU: the host side of the weight container (kokorox_amd/csrc/kxw_file.cpp: kxw_header, kxw_table, read_weight_file).

The table decides every weight pointer a kernel reads, and Model::build and the forward hard-code the architecture, so a
table is accepted in one place and only if it is sound (aligned, in range without wrap-around, consistent sizes, no name
twice, nothing inside the table) AND holds every tensor of tensor_spec() with the spec's shape.  Checked here without a GPU
and without loading anything into python: tests/cpp/kxw_fuzz.cpp is built with g++ -fsanitize=address,undefined together
with kxw_file.cpp and onnx_import.cpp and run as a child process.  A table needs no tensor data, so the driver works on the
header and table alone (about 64 KB) and is told the container's size.
"""
import importlib.util
import os
import shutil
import struct
import subprocess

import pytest

from kokorox_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM_BIAS = "predictor.lstm.bias_ih_l0"  # [1024], 4096 bytes: the tensor the directed cases (and the GPU cases) damage
_FIELDS = {"dtype": (88, "<I"), "ndim": (92, "<I"), "offset": (112, "<Q"), "nbytes": (120, "<Q")}


# ---- helpers shared with tests/test_gpu_importer.py -------------------------------------------------------------------------
def table_image(spec=None):
    """(header + table of the container W.write_blob would write for `spec`, with no data; its layout; its total_bytes)"""
    table, data_off, total = W._layout(spec or W.tensor_spec())
    img = bytearray(W.MAGIC + struct.pack("<IIQQ", len(table), len(table) * W.ENTRY_BYTES, data_off, total)).ljust(64, b"\0")
    for name, shape, off, nbytes in table:
        dims = list(shape) + [0] * (4 - len(shape))
        img += name.encode().ljust(W.NAME_BYTES, b"\0") + struct.pack("<II4IQQ", 0, len(shape), *dims, off, nbytes)
    assert len(img) == 64 + len(table) * W.ENTRY_BYTES
    return img, table, total


def entry_at(buf, name):
    """byte position of the table entry called `name` in a container (or its header + table) held in a writable buffer"""
    mv = memoryview(buf).cast("B")
    (n,) = struct.unpack_from("<I", mv, 8)
    want = name.encode().ljust(W.NAME_BYTES, b"\0")
    for i in range(n):
        at = 64 + i * W.ENTRY_BYTES
        if bytes(mv[at: at + W.NAME_BYTES]) == want:
            return at
    raise KeyError(name)


def patch_entry(buf, name, *, new_name=None, dims=None, **fields):
    """Change fields of ONE table entry in place: new_name (bytes, at most 88), dims (1 to 4 values; ndim is not touched),
    dtype, ndim, offset, nbytes.  Works on a bytearray and on a numpy uint8 array."""
    mv = memoryview(buf).cast("B")
    at = entry_at(buf, name)
    if new_name is not None:
        assert len(new_name) <= W.NAME_BYTES
        mv[at: at + W.NAME_BYTES] = new_name.ljust(W.NAME_BYTES, b"\0")
    if dims is not None:
        struct.pack_into(f"<{len(dims)}I", mv, at + 96, *dims)
    for k, v in fields.items():
        off, fmt = _FIELDS[k]
        struct.pack_into(fmt, mv, at + off, v)


def shrink_lstm_bias(buf):
    """`predictor.lstm.bias_ih_l0` as [1023] / 4092 bytes, offset and data untouched: consistent, aligned and in range, but not
    the model's shape.  (The tensor's 256-byte padding covers the four bytes a 1024-float read would take.)"""
    patch_entry(buf, LSTM_BIAS, dims=[1023], nbytes=4092)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kxw_fuzz") / "kxw_fuzz")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "kxw_fuzz.cpp"), os.path.join(csrc, "kxw_file.cpp"),
                    os.path.join(csrc, "onnx_import.cpp"), "-o", exe], check=True)

    def run(*args, env=None):
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        e.pop("KOKOROX_KXW_CACHE", None)
        e.update(env or {})
        r = subprocess.run([exe, *map(str, args)], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


def test_the_writers_table_is_accepted_as_written(driver, tmp_path):
    img, table, total = table_image()
    p = tmp_path / "table.kxw"
    p.write_bytes(img)
    got = {}
    for line in driver("dump", total, p).splitlines():
        name, *nums = line.split(" ")
        nd, d0, d1, d2, d3, off, nb = map(int, nums)
        got[name] = ((d0, d1, d2, d3)[:nd], off, nb)
    assert got == {name: (tuple(shape), off, nb) for name, shape, off, nb in table}


def _directed_cases():
    """name -> (one change to the table, what the message must contain)"""
    img, table, total = table_image()
    _, shape, off, nb = next(t for t in table if t[0] == LSTM_BIAS)
    assert (shape, nb, off % 256) == ((1024,), 4096, 0)
    at = entry_at(img, LSTM_BIAS)
    assert at + 2 * W.ENTRY_BYTES <= len(img)

    def twice(b):  # the entry behind it becomes a copy of it
        b[at + W.ENTRY_BYTES: at + 2 * W.ENTRY_BYTES] = b[at: at + W.ENTRY_BYTES]

    def raise_n(b):
        struct.pack_into("<I", b, 8, len(table) + 1)

    long_name = (LSTM_BIAS + "_").encode().ljust(W.NAME_BYTES, b"x")
    cases = {
        "offset_wraps": (lambda b: patch_entry(b, LSTM_BIAS, offset=2 ** 64 - 256), ["bad entry", LSTM_BIAS]),
        "ends_256_past_total": (lambda b: patch_entry(b, LSTM_BIAS, offset=total + 256 - nb), ["bad entry", LSTM_BIAS]),
        "misaligned": (lambda b: patch_entry(b, LSTM_BIAS, offset=off + 4), ["bad entry", LSTM_BIAS]),
        "inside_the_table": (lambda b: patch_entry(b, LSTM_BIAS, offset=64), ["bad entry", LSTM_BIAS]),
        "count_wraps": (lambda b: patch_entry(b, LSTM_BIAS, ndim=4, dims=[2 ** 31, 2 ** 31, 4, 1], nbytes=0), ["size mismatch", LSTM_BIAS]),
        "ndim_5": (lambda b: patch_entry(b, LSTM_BIAS, ndim=5), ["bad entry", LSTM_BIAS]),
        "dtype_1": (lambda b: patch_entry(b, LSTM_BIAS, dtype=1), ["bad entry", LSTM_BIAS]),
        "not_the_models_shape": (shrink_lstm_bias, ["shape mismatch", LSTM_BIAS, "[1023]", "[1024]"]),
        "name_off_by_a_letter": (lambda b: patch_entry(b, LSTM_BIAS, new_name=LSTM_BIAS[:-1].encode() + b"1"), ["missing tensor " + LSTM_BIAS]),
        "entry_twice": (twice, ["bad entry", LSTM_BIAS, "twice"]),
        "name_without_nul": (lambda b: patch_entry(b, LSTM_BIAS, new_name=long_name), ["bad entry", long_name.decode()]),
        "one_tensor_too_many": (raise_n, ["truncated tensor table"]),
        "header_of_63_bytes": (lambda b: b.__delitem__(slice(63, None)), ["bad magic"]),
    }
    return img, total, cases


def test_directed_cases_are_refused_with_io_status_and_the_tensors_name(driver, tmp_path):
    img, total, cases = _directed_cases()
    paths = []
    for name, (change, _) in cases.items():
        b = bytearray(img)
        change(b)
        assert b != img, name
        p = tmp_path / f"{name}.kxw"
        p.write_bytes(b)
        paths.append(p)
    lines = driver("check", total, *paths).splitlines()
    assert len(lines) == len(cases)
    for (name, (_, needles)), line in zip(cases.items(), lines):
        assert line.startswith("error 2 weight blob: "), f"{name}: {line}"
        for s in needles:
            assert s in line, f"{name}: {line}"


def test_table_fuzz_under_address_and_ub_sanitizers(driver, tmp_path):
    """20 000 mutations of the header and table from a fixed seed, each in a heap buffer of exactly its length: an accepted
    table or kx::Error(KX_ERR_IO), anything else is a sanitizer report.  No ratio is asserted (a flip in a reserved byte or in
    the name padding is legitimately accepted)."""
    img, _, total = table_image()
    p = tmp_path / "table.kxw"
    p.write_bytes(img)
    out = driver("fuzz", total, p, 20000, 1)
    print(out)
    words = out.split()
    assert "mutations" in out
    accepted, rejected = int(words[words.index("accepted,") - 1]), int(words[words.index("rejected") - 1])
    assert accepted + rejected == 20001
    assert accepted >= 1 and rejected >= 1  # (the driver itself fails when the unmutated table is not accepted)


# ---- read_weight_file ----------------------------------------------------------------------------------------------------------
def _cases_module():
    p = os.path.join(ROOT, "tests", "test_onnx_cpp_cpu.py")
    spec = importlib.util.spec_from_file_location("_onnx_cpp_cases", p)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_cpp = _cases_module()
synth = _cpp.synth  # (module-scoped fixtures of test_onnx_cpp_cpu.py: the exporter-style model_<style>.onnx files)
files = _cpp.files


def _read(driver, path, cache=None):
    out = driver("read", path, env={"KOKOROX_KXW_CACHE": cache} if cache else None).strip()
    if out.startswith("error"):
        return out
    w = out.split()
    return {"variant": int(w[1]), "bytes": int(w[3]), "fnv1a": w[5]}


def test_read_weight_file_converts_and_caches_only_when_asked(driver, files, tmp_path):
    src = str(tmp_path / "model.onnx")
    shutil.copyfile(files["fp32"], src)
    cache, stamp = src + ".kxw", src + ".kxw.src"
    first = _read(driver, src)
    assert first["variant"] == 1 and first["bytes"] == W._layout(W.tensor_spec())[2]
    assert sorted(os.listdir(tmp_path)) == ["model.onnx"], "nothing may be written beside the source unasked"
    a = _read(driver, src, cache="1")
    assert a == first
    assert sorted(os.listdir(tmp_path)) == ["model.onnx", "model.onnx.kxw", "model.onnx.kxw.src"]
    assert os.path.getsize(cache) == first["bytes"]
    b = _read(driver, src, cache="1")
    assert b == dict(first, variant=-1), "the second read is the cache, with the same bytes"
    assert _read(driver, src, cache="yes") == first, "only KOKOROX_KXW_CACHE=1 is the switch"
    # a stamp that differs in one character: converted again (and the stamp rewritten)
    good = open(stamp).read()
    assert good.startswith("kxw-cache 1 importer 1 size %d mtime " % os.path.getsize(src)) and good.endswith("\n")
    with open(stamp, "w") as f:
        f.write(good.replace("importer 1", "importer 2"))
    assert _read(driver, src, cache="1") == first
    assert open(stamp).read() == good
    # a cache file cut by one byte is ignored
    with open(cache, "r+b") as f:
        f.truncate(first["bytes"] - 1)
    assert _read(driver, src, cache="1") == first
    assert os.path.getsize(cache) == first["bytes"]
    assert not [n for n in os.listdir(tmp_path) if ".tmp" in n]


def test_read_weight_file_refuses_a_wrong_size_and_a_missing_path(driver, tmp_path):
    img, _, total = table_image()
    p = tmp_path / "short.kxw"
    p.write_bytes(img)  # (the header says total_bytes, the file ends with the table)
    assert len(img) != total
    assert _read(driver, p) == "error 2 weight blob: file size does not match header"
    out = _read(driver, tmp_path / "absent.kxw")
    assert out.startswith("error 2 cannot open weight file: ") and out.endswith("absent.kxw")
