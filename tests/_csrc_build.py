"""What the CPU tests ask of modulate_amd/csrc's build: `make`'s own answers (a variable's value, the plan of a target), the one
loader of check_isa.py, and the one way a san_*_cases.py file is run against the sanitizer builds of the library's host code."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modulate_amd", "csrc")


def _assignments(overrides):
    return [f"{k}={v}" for k, v in overrides.items()]


def make_var(name, **overrides):
    """The expanded value of a Makefile variable.  (With ISA_CHECK="0" among the overrides the Makefile's "NOT checked" notice, printed
    while it is read, comes first in the answer.)"""
    r = subprocess.run(["make", "-s", "-C", CSRC, "--eval", f"print-var: ; @echo $({name})", "print-var"] + _assignments(overrides),
                       capture_output=True, text=True, check=True)
    return r.stdout.strip()


def dry_run(*targets, **overrides):
    """The lines `make` would run to remake `targets` from nothing (and what it prints while reading the Makefile)."""
    r = subprocess.run(["make", "-n", "-B", "-C", CSRC, *targets] + _assignments(overrides), capture_output=True, text=True, check=True)
    return r.stdout.splitlines()


def guard_then_compile(tu, asm=None):
    """The object of `tu` waits for its guard: in the plan of <tu>.o the check_isa.py run over `asm` (default: the TU's own
    assembly) comes before the compile.  Returns the plan."""
    plan = dry_run(tu + ".o")
    guard = "python3 check_isa.py " + (asm or tu + ".s")
    assert guard in plan, plan
    compile_at = next(i for i, ln in enumerate(plan) if f" -c {tu}.hip " in ln)
    assert plan.index(guard) < compile_at, plan
    return plan


def unguarded_plan(tu):
    """ISA_CHECK=0 leaves the guard out: no check_isa.py run in the plan of <tu>.o and no stamp touched; the object is still built."""
    plan = dry_run(tu + ".o", ISA_CHECK="0")
    assert not any("check_isa.py" in ln or ln.startswith("touch") for ln in plan), plan
    assert any(f" -c {tu}.hip " in ln for ln in plan), plan
    return plan


def standin_is_wired(name):
    """tests/cpu_runtime_standin/<name> is a source of both sanitizer builds of the library."""
    lines = [ln for ln in dry_run("sanitize-lib") if ln.startswith("g++ ") and " -fsanitize=" in ln]
    assert len(lines) == 2 and all(f"/cpu_runtime_standin/{name} " in ln for ln in lines), lines


def isa_check_target(target, kernels):
    """`make <target>` passes the tree and prints its one line, with the TU's own kernel count."""
    r = subprocess.run(["make", "-s", "-C", CSRC, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("check_isa:")] == [f"check_isa: ok ({kernels} kernels)"], r.stdout


def load_check_isa():
    spec = importlib.util.spec_from_file_location("check_isa", os.path.join(CSRC, "check_isa.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sanitizer_runtime(name):
    p = subprocess.run(["gcc", f"-print-file-name={name}"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def run_sanitized_cases(case_file, flavour, expect, extra_env=(), drop_env=("MODGPU_DEVICE_ALIAS", "MODGPU_SHIM_SLOW"), select=()):
    """tests/<case_file> in a child pytest against the `flavour` ("asan": ASan + UBSan, "tsan") build of the library's host code
    (`make sanitize-lib`).  Skips when gcc's runtime for the flavour is not installed."""
    import pytest
    if flavour == "asan":
        asan, ubsan = sanitizer_runtime("libasan.so"), sanitizer_runtime("libubsan.so")
        if not asan or not ubsan:
            pytest.skip("gcc sanitizer runtimes not installed")
        preload = f"{asan}:{ubsan}"
        options = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
    else:
        preload = sanitizer_runtime("libtsan.so")
        if not preload:
            pytest.skip("gcc ThreadSanitizer runtime not installed")
        options = {"TSAN_OPTIONS": f"halt_on_error=1 second_deadlock_stack=1 suppressions={os.path.join(ROOT, 'tests', 'tsan.supp')}"}
    from oracle import oracle as O
    O.build(ref=False)  # here, not in the child: the compiler must not run under a preloaded sanitizer runtime
    subprocess.check_call(["make", "-s", "-C", CSRC, "sanitize-lib"])
    env = dict(os.environ, LD_PRELOAD=preload, MODGPU_LIB=os.path.join(ROOT, "modulate_amd", "_san", f"libmodgpu_{flavour}.so"),
               MODGPU_SHIM_DEVICES="8", MODGPU_REQUIRE_GPU="0", **options, **dict(extra_env))
    for k in drop_env:
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", case_file), "-x", "-q", "-p", "no:cacheprovider"] + list(select),
                       env=env, capture_output=True, text=True, cwd=ROOT, timeout=1500)
    assert r.returncode == 0 and expect in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
