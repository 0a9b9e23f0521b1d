"""CPU: the dispatcher's host logic for requests of several chunks under ThreadSanitizer and AddressSanitizer + UBSan, built
and run exactly as tests/test_host_sanitize_cpu.py runs its scenarios (g++; kokorox_amd/csrc/dispatcher_core.h is HIP-free).

The reference runs a text's chunks one after the other through its one `Mutex<Session>`
(/root/reference/kokorox/src/tts/koko.rs:947-1191); here a request of n chunks is n rows of one batched forward.
tests/cpp/request_sanitize.cpp drives a stub model that understands rows: 64 client threads mixing single rows with requests of
2..max_batch chunks, batches counted in rows, no request split over forwards, a max_batch-chunk request behind a stream of small
ones, INVALID replay of whole requests, re-queue from a failed model, chunk counts refused at submit, destroy-while-queued."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,flags,env", [
    ("thread", ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1"}),
    ("address", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
     {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1"}),
])
def test_multi_chunk_requests_under_sanitizers(tmp_path, name, flags, env):
    exe = str(tmp_path / f"request_{name}")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "kokorox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "request_sanitize.cpp"), "-o", exe, "-lpthread"], check=True)
    for _ in range(3):  # (thread interleavings differ from run to run)
        r = subprocess.run([exe], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "scenarios passed" in r.stdout, r.stdout[-1000:] + r.stderr[-6000:]
        assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr
