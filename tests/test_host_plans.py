"""What the C ABI decides on the host, checked on the CPU: the engine a program gets (dusp_amd/csrc/engine_select.hpp), the small launch
decisions of a render (render_plan.hpp), and the registry of a program's device workspaces (abi_internal.hpp).  Each is a stand-alone
program under tests/native, built with AddressSanitizer + UBSan."""
import glob
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SANITIZE = ["-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Wno-unused-parameter"]


def _build_and_run(tmp_path, name, args=(), flags=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + SANITIZE + list(flags) + ["-o", exe, os.path.join(NATIVE, name + ".cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    out, err = p.stdout.decode(), p.stderr.decode()
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (out[-4000:], err[-4000:])
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0, out[-4000:]
    return rep


def test_engine_selection_follows_its_rules_for_every_golden_descriptor(tmp_path):
    """engine_select over every golden descriptor x requested engine {AUTO, CHUNK, FUSED, WAVE} x {plain, resumable}, as new programs (compiled
    kernels on and off, a context whose tables the sum chain does not take) and as continuations (engine so far, a Delay's constant changed),
    against the rules written out in the check as a table over plan_fused / plan_wave / jit_eligible called on their own: AUTO takes the first
    engine that applies; a forced engine that does not apply is DUSP_ERR_UNSUPPORTED with the build's text; a resumable program with rings or
    feedback goes to wave if plannable, else chunk, and is refused on FUSED; a continuation stays on wave, falls to chunk when a Delay
    changed, and falls back to AUTO's rules where its forced engine stopped applying; a hand-off only under AUTO, plain, no inputs, compiled
    kernels on.  The counters say that every rule was met by cases."""
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.desc.f64")))
    assert len(files) >= 200
    rep = _build_and_run(tmp_path, "engine_select_check", files)
    assert rep["files"] == len(files) and rep["cases"] >= 50 * len(files), rep
    assert rep["auto_fused"] > 0 and rep["auto_wave"] > 0 and rep["auto_chunk"] > 0 and rep["refused"] > 0, rep
    assert rep["resumable_wave"] > 0 and rep["resumable_chunk"] > 0 and rep["resumable_refused"] > 0, rep
    assert rep["delay_stays_wave"] > 0 and rep["delay_falls_to_chunk"] > 0 and rep["feed_forward_stays_wave"] > 0 and rep["back_to_auto"] > 0, rep
    assert rep["handoff"] > 0 and rep["jit"] > 0 and rep["fx32"] > 0, rep


def test_render_plan_boundary_values(tmp_path):
    """The sum chain's blocks of groups, the default tile of a mix and a hand-off's warm-up chunks at the values where each rule turns."""
    rep = _build_and_run(tmp_path, "render_plan_check")
    assert rep["cases"] >= 24, rep


def test_jump_ahead_integer_helpers_and_the_sum_chains_block_base_are_exact(tmp_path):
    """dusp_amd/csrc/modmath.hpp against unsigned __int128: addmod, mulmod, mod_u32, mod_u64 and jit_mulmod at every modulus in use
    (sampleRate << 32 and << 36 over the sample-rate matrix, 2^17) with operands at their edges, the sum chain's block base for every
    block count a launch can have — among them the ones whose plain 64-bit product passes 2^64 — and a voice's record from
    build_sum_voices to the phase of a sample for windows up to sample 2^40."""
    rep = _build_and_run(tmp_path, "sumchain_base_check")
    assert rep["cases"] >= 100000 and rep["mod_u64"] >= 1500 and rep["mod_u32"] >= 300 and rep["jit_mulmod"] >= 10000, rep
    assert rep["block_base"] >= 7000 and rep["block_base_int"] >= 800 and rep["voice_phases"] >= 100000 and rep["products_past_2_64"] >= 500, rep


def test_workspace_registry_names_every_overwritten_guard(tmp_path):
    """Every DevBuf of a program is in the registry its destructor and the guard check walk: with "device" memory on the host
    (tests/native/hip_mem_stub), a byte flipped behind each workspace in turn is reported under that workspace's name.  The header's shared argument checks give every entry point the text it has always given."""
    rep = _build_and_run(tmp_path, "workspace_registry_check", flags=["-I" + os.path.join(NATIVE, "hip_mem_stub")])
    assert rep["workspaces"] >= 28 and rep["flips"] == 3 * rep["workspaces"] and rep["texts"] >= 20, rep
