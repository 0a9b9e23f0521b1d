"""CPU: what a call is refused for before it touches the device, and where its output bytes go
(kokorox_amd/csrc/host_request.cpp: check_host_call, check_device_call, build_output_plan, output_bounds).

Model::infer_host_once and Model::infer_device take their argument checks and the layout of the compact output from that unit,
which includes no HIP header: tests/cpp/host_request_check.cpp is built with g++ -fsanitize=address,undefined together with it
and run as a child process.  Nothing is loaded into python.  The messages are the library's interface as much as the codes are
(callers and the GPU suite match on them), so every refusal is pinned to its exact text, and the two entries' different wordings
of the same violation stay apart.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NULL_OUT = "infer: null output argument"
NULL_ARG = "infer: null argument"
FORMAT = "infer: unknown output format"
KIND_FORMAT = "infer: unknown kind / output format"
MIX = "infer: voice table not set or bad mix"
TOKENS = "infer: token count must be 1..512"
TOKEN_ID = "infer: token id outside 0..177"
CHUNKS = "infer: chunks_per_request entries must be >= 1 and add up to the batch"
NO_VOICE = "infer: no voice given"
BATCH = "infer: batch must be 1..4096 (empty input is an error)"
SPEED = "infer: speed must be > 0"

HOST_REFUSALS = {
    "null_out": NULL_OUT, "null_out_bytes": NULL_OUT, "null_out_samples": NULL_OUT,
    "B_0": "infer: empty batch",
    "null_ids": NULL_ARG, "null_lens": NULL_ARG, "null_speeds": NULL_ARG,
    "format_3_ungrouped": FORMAT,
    "utt_index_without_seeds": "infer: utterance indices go with per-row seeds",
    "neither_styles_nor_voices": "infer: styles or voice ids are required",
    "kinds_with_styles_only": "infer: per-utterance kinds need both styles and voice ids",
    "kinds_with_voices_only": "infer: per-utterance kinds need both styles and voice ids",
    "voices_without_table": MIX, "voices_without_weights": MIX, "max_mix_0": MIX, "max_mix_17": MIX,
    "lens_0": TOKENS, "lens_513": TOKENS, "lens_above_stride": TOKENS,
    "id_minus_1": TOKEN_ID, "id_n_vocab": TOKEN_ID,
    "kind_3": KIND_FORMAT,
    "voice_row_of_one_token": "infer: voice rows need the two 0 pads (row = tokens - 2)",
    "voice_id_n_voices": "infer: voice id outside the table",
    "all_voice_ids_negative": NO_VOICE, "kind_1_negative_first_id": NO_VOICE,
}
# the eight (chunks_per_request, format) pairs of tests/test_gpu_wire_formats.py::test_model_refuses_bad_groupings_and_formats
BAD_GROUPINGS = {
    "grouped_1_2_format_5": FORMAT, "grouped_1_2_formats_0_5": FORMAT, "grouped_1_2_format_minus_1": FORMAT,
    "grouped_1_0_2": CHUNKS, "grouped_1_1": CHUNKS, "grouped_2_2": CHUNKS, "grouped_3_1": CHUNKS,
    "grouped_1_2_formats_0_1_2": "infer: requests need 1 or R output formats",
}
HOST_ACCEPTED = ["ok_style_rows", "ok_style_rows_seeds_and_index", "ok_single_voice", "ok_mix", "ok_per_utterance_kinds",
                 "ok_ungrouped_each_form", "ok_grouped_shared_format", "ok_grouped_formats_per_request"]
DEVICE_REFUSALS = {
    "B_0": BATCH, "B_4097": BATCH,
    "null_ids": NULL_ARG, "null_styles": NULL_ARG,
    "n_speed_2_of_3": "infer: n_speed must be 1 or B",
    "lens_0": TOKENS, "lens_513": TOKENS,
    "lens_above_stride": "infer: lens[b] exceeds the row stride",  # (the host entry's wording: TOKENS)
    "speed_0": SPEED, "speed_negative": SPEED,
}
DEVICE_ACCEPTED = ["ok_one_speed", "ok_speed_per_row", "ok_B_4096"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_request") / "host_request_check")
    csrc = os.path.join(ROOT, "kokorox_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                    os.path.join(ROOT, "tests", "cpp", "host_request_check.cpp"), os.path.join(csrc, "host_request.cpp"),
                    "-o", exe], check=True)

    def run(mode):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, mode], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


@pytest.fixture(scope="module")
def outcomes(driver):
    got = {}
    for line in driver("refusals").splitlines():
        name, *rest = line.split("\t")
        assert name not in got, name
        got[name] = tuple(rest)
    return got


def test_every_case_of_the_driver_is_expected_here(outcomes):
    want = {"host." + k for k in (*HOST_REFUSALS, *BAD_GROUPINGS, *HOST_ACCEPTED)} | {"device." + k for k in (*DEVICE_REFUSALS, *DEVICE_ACCEPTED)}
    assert set(outcomes) == want


def test_host_entry_refusals_have_code_1_and_their_exact_message(outcomes):
    for name, msg in HOST_REFUSALS.items():
        assert outcomes["host." + name] == ("1", msg), name


def test_bad_groupings_and_formats_are_refused_without_a_device(outcomes):
    for name, msg in BAD_GROUPINGS.items():
        assert outcomes["host." + name] == ("1", msg), name


def test_one_call_of_each_kind_is_accepted(outcomes):
    for name in HOST_ACCEPTED:
        assert outcomes["host." + name] == ("accepted",), name
    for name in DEVICE_ACCEPTED:
        assert outcomes["device." + name] == ("accepted",), name


def test_device_entry_refusals_keep_their_own_wording(outcomes):
    for name, msg in DEVICE_REFUSALS.items():
        assert outcomes["device." + name] == ("1", msg), name
    assert outcomes["host.lens_above_stride"][1] != outcomes["device.lens_above_stride"][1]


def test_layout_request_plans_and_the_packed_bound(driver):
    """The plan of a per-utterance call (B = 5 single-row requests, frames 1 7 422 1 3, forms all 0 / 1 / 2 through a null
    grouping and mixed through a grouped call), the request plan of every composition
    of 6 rows with each form shared and one mixed assignment, the bound of 1..64 one-frame requests in every form, and the
    sample count from which a 16-bit WAV file is refused: the driver compares with sums written out on its own."""
    out = driver("layout")
    print(out)
    assert "utterance layout: 4 assignments of forms over 5 utterances" in out
    assert "request plans: 192 (composition, forms) pairs over 6 rows" in out
    assert "bounds: 64 x 5 one-frame batches; form 4 refused from 2147483630 samples" in out
