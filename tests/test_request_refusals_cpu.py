"""CPU: what the request options are refused for, word for word, and which refusal wins when two arguments are wrong at once.

The host entry's checks (kokorox_amd/csrc/host_request.cpp) and every submit_request* of the dispatcher on a stub model, built with
g++ -fsanitize=address,undefined into tests/cpp/request_refusals_check.cpp and run as a child process.  The expected texts are
written out here, not taken from the library: they are what callers match on, and what any re-threading of the arguments between
the C entries and the forward has to keep.
"""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kokorox_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("request_refusals") / "request_refusals_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "request_refusals_check.cpp"),
                    os.path.join(CSRC, "host_request.cpp"), "-lpthread", "-o", exe], check=True)

    def run(mode):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        r = subprocess.run([exe, mode], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]  # (a sanitizer report aborts the driver)
        return r.stdout
    return run


# ---- the host entry ---------------------------------------------------------------------------------------------------------------
BAD_SPECS = {
    "join": ["flags_8", "keep_-1", "keep_1001", "pause_-1", "pause_5001", "fade_-1", "fade_13"],
    "level": ["mode_3", "mode_0x200", "gain_-0.5", "gain_65", "gain_nan", "peak_in_mode_0", "gain_in_mode_1", "peak_0", "peak_2", "peak_nan"],
    "loudness": ["mode_2", "mode_none", "target_in_mode_0", "peak_in_mode_0", "target_-71", "target_1", "target_nan", "peak_0", "peak_2",
                 "peak_nan"],
    "limit": ["mode_2", "mode_none", "gain_-0.5", "gain_65", "gain_nan", "target_in_mode_0", "gain_in_mode_1", "target_1", "target_nan",
              "peak_0", "peak_2", "peak_nan"],
}
BAD_PROSODY = ["rate_0.2", "rate_5", "rate_nan", "frames_-1", "frames_51", "pitch_0.2", "pitch_5", "pitch_nan", "energy_-1", "energy_5",
               "energy_nan"]
# the checks in the order the host entry runs them, each with the refusal of its argument left null
HOST_ORDER = [("output", "infer: null output argument"), ("join", "infer: null join argument"), ("marks", "infer: null marks argument"),
              ("level", "infer: null level argument"), ("loudness", "infer: null loudness argument"), ("limit", "infer: null limit argument"),
              ("prosody", "infer: null report argument")]


def test_host_entry_refusals_word_for_word_and_in_order(driver):
    got = dict(line.split("\t", 1) for line in driver("host").splitlines())
    want = {}
    for noun, bad in BAD_SPECS.items():
        want[f"{noun}.null"] = f"1\tinfer: null {noun} argument"
        want[f"{noun}.count_0"] = f"1\tinfer: bad {noun} count"
        want[f"{noun}.count_3_and_bad"] = f"1\tinfer: bad {noun} count"
        want[f"{noun}.shared_ok"] = want[f"{noun}.per_request_ok"] = "accepted"
        for name in bad + ["second_bad"]:
            want[f"{noun}.{name}"] = f"1\tinfer: bad {noun}"
    assert want["join.null"] == "1\tinfer: null join argument" and want["loudness.count_0"] == "1\tinfer: bad loudness count"
    assert want["limit.peak_nan"] == "1\tinfer: bad limit" and want["level.second_bad"] == "1\tinfer: bad level"
    want.update({"marks.ok": "accepted", "marks.null_marks": "1\tinfer: null marks argument",
                 "marks.null_count": "1\tinfer: null marks argument",
                 "marks.not_grouped": "1\tinfer: marks are for requests (chunks_per_request)"})
    want.update({"prosody.null_spec_ok": "accepted", "prosody.no_report_ok": "accepted", "prosody.all_edges_ok": "accepted",
                 "prosody.null_report": "1\tinfer: null report argument", "prosody.null_count": "1\tinfer: null report argument",
                 "prosody.reports_without_the_pair": "1\tinfer: reports are for requests (chunks_per_request)",
                 "prosody.reports_not_grouped": "1\tinfer: reports are for requests (chunks_per_request)",
                 "prosody.null_count_and_rate_5": "1\tinfer: null report argument"})
    for name in BAD_PROSODY:
        want[f"prosody.{name}"] = "1\tinfer: bad prosody"
    for (a, text), (b, _) in itertools.combinations(HOST_ORDER, 2):
        want[f"both.{a}+{b}"] = "1\t" + text
    assert got == want


def test_the_driver_runs_the_checks_in_the_order_of_the_host_entry():
    """The driver repeats the check sequence of Model::infer_host_once (which needs a GPU); the two are held together here."""
    def sequence(path, start):
        text = open(path, encoding="utf-8").read()
        body = text[text.index(start):]
        return re.findall(r"^ *if \(hc\.([\w.]+)\) (?:kx::)?check_", body[:body.index("\n}\n")], re.M)
    want = ["joins.call", "req_marks", "levels.call", "loudness.call", "limits.call", "prosody_call"]
    assert sequence(os.path.join(CSRC, "model_host.hip"), "void Model::infer_host_once(") == want
    assert sequence(os.path.join(ROOT, "tests", "cpp", "request_refusals_check.cpp"), "void host_checks(") == want


# ---- the dispatcher's submits -----------------------------------------------------------------------------------------------------
WHO = "dispatcher_submit_request: "
CHUNKS = WHO + "a request has 1..8 chunks (max_batch)"
TOKENS = WHO + "chunk 0: 1..512 tokens (with a voice: at least the two 0 pads)"
# per entry: what it can be given wrong, in the order in which it looks, and the refusal; None = that state of the argument is accepted
SUBMITS = {
    "request": [("null_out", WHO + "null output argument"), ("chunks", CHUNKS), ("tokens", TOKENS)],
    "marks": [("null_out", WHO + "null output argument"), ("marks_half", WHO + "null marks argument"), ("marks_null", WHO + "null marks argument"),
              ("chunks", CHUNKS), ("tokens", TOKENS)],
    "joined": [("bad_join", WHO + "bad join"), ("null_join", WHO + "bad join"), ("null_out", WHO + "null output argument"),
               ("marks_half", WHO + "null marks argument"), ("marks_null", None), ("chunks", CHUNKS), ("tokens", TOKENS)],
    "levelled": [("bad_join", WHO + "bad join"), ("null_join", None), ("bad_spec", WHO + "bad level"), ("null_spec", WHO + "bad level"),
                 ("null_out", WHO + "null output argument"), ("marks_half", WHO + "null marks argument"), ("marks_null", None),
                 ("chunks", CHUNKS), ("tokens", TOKENS)],
    "loudness": [("bad_join", WHO + "bad join"), ("null_join", None), ("bad_spec", WHO + "bad loudness"), ("null_spec", WHO + "bad loudness"),
                 ("null_out", WHO + "null output argument"), ("marks_half", WHO + "null marks argument"), ("marks_null", None),
                 ("chunks", CHUNKS), ("tokens", TOKENS)],
    "limited": [("bad_join", WHO + "bad join"), ("null_join", None), ("bad_spec", WHO + "bad limit"), ("null_spec", WHO + "bad limit"),
                ("null_out", WHO + "null output argument"), ("marks_half", WHO + "null marks argument"), ("marks_null", None),
                ("chunks", CHUNKS), ("tokens", TOKENS)],
    "prosody": [("bad_join", WHO + "bad join"), ("null_join", None), ("null_spec", None), ("report_half", WHO + "null report argument"),
                ("null_out", WHO + "null output argument"), ("marks_half", WHO + "null marks argument"), ("marks_null", None),
                ("chunks", CHUNKS), ("tokens", TOKENS), ("bad_prosody", WHO + "bad prosody")],
}
EXCLUSIVE = [{"bad_join", "null_join"}, {"bad_spec", "null_spec"}, {"marks_half", "marks_null"}, {"null_spec", "bad_prosody"}]
# the driver names the faults of a pair in this order
NAMES = ["bad_join", "null_join", "bad_spec", "null_spec", "report_half", "marks_half", "marks_null", "null_out", "chunks", "tokens",
         "bad_prosody"]


def test_every_submit_refuses_the_same_words_and_the_same_argument_first(driver):
    got = {}
    for line in driver("dispatcher").splitlines():
        entry, faults, rest = line.split("\t", 2)
        assert (entry, faults) not in got
        got[(entry, faults)] = rest
    want = {}
    for entry, order in SUBMITS.items():
        want[(entry, "none")] = "accepted"
        singles = [(name,) for name, _ in order]
        pairs = [p for p in itertools.combinations([n for n in NAMES if n in dict(order)], 2) if set(p) not in EXCLUSIVE]
        for faults in singles + pairs:
            texts = [text for name, text in order if name in faults and text is not None]  # (in the order the entry looks)
            want[(entry, "+".join(faults))] = "1\t" + texts[0] if texts else "accepted"
    # a bad join wins over a null output argument, and the joined entry alone refuses a null join
    assert want[("limited", "bad_join+null_out")] == "1\tdispatcher_submit_request: bad join"
    assert want[("joined", "null_join")] == "1\tdispatcher_submit_request: bad join" and want[("prosody", "null_join")] == "accepted"
    assert want[("marks", "marks_half+null_out")] == "1\tdispatcher_submit_request: null output argument"
    assert got == want
