"""CPU: the launchers' grid, tile-count, column-chunk and measurement-knob rules (csrc/sf_launch_plan.h), away from any device.  tests/launch_plan_main.cpp
is built with the host C++ compiler under the address and undefined-behaviour sanitizers and run; every line it prints is compared with the formula the
launchers carried, written out, before the header existed - those formulas, copied here literally, are the oracle, not the header."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
N_CUS = (1, 7, 8, 9, 255, 256, 304)
ITEMS = (1, 7, 8, 9, 255, 256, 257, 2 ** 31 - 1)


def _xcd_grid(n_cu, total):
    # launch_gemm_persistent and eight more: `int64_t blocks = (n_cu / 8) * 8; if (blocks < 8) blocks = 8; need = ((total + 7) / 8) * 8; if (blocks > need) blocks = need;`
    blocks = (n_cu // 8) * 8
    if blocks < 8:
        blocks = 8
    need = ((total + 7) // 8) * 8
    if blocks > need:
        blocks = need
    return blocks


def _xcd_grid_uncapped(n_cu):
    # sf_gemm_tn_pp: `int64_t blocks = n_cu & ~7; if (blocks < 8) blocks = 8;`
    blocks = n_cu & ~7
    if blocks < 8:
        blocks = 8
    return blocks


def _cu_grid(n_cu, tiles):
    # sf_gemm_res_ln768 and two more: `tiles < n_cu ? tiles : n_cu`
    return tiles if tiles < n_cu else n_cu


def _tile_counts(M, N, BM, BN):
    # `tiles_m = (M + BM - 1) / BM; tiles_n = (uint32_t)((N + BN - 1) / BN); total = tiles_m * tiles_n; if (total >= ((int64_t)1 << 31)) -> "too many tiles"`
    tiles_m = (M + BM - 1) // BM
    tiles_n = ((N + BN - 1) // BN) & 0xffffffff
    total = tiles_m * tiles_n
    if total >= (1 << 31):
        return None
    return tiles_n, total


def _nchunk_bf16(K):
    # `a.K <= 1024 ? (uint32_t)(2400000 / (512 * a.K) > 0 ? 2400000 / (512 * a.K) : 1) : 0u`
    return (2400000 // (512 * K) if 2400000 // (512 * K) > 0 else 1) if K <= 1024 else 0


def _nchunk_mxfp8(K):
    # `a.K <= 2048 ? (uint32_t)(2400000 / (256 * a.K) > 0 ? 2400000 / (256 * a.K) : 1) : 0u`
    return (2400000 // (256 * K) if 2400000 // (256 * K) > 0 else 1) if K <= 2048 else 0


def _expected():
    out = []
    for n_cu in N_CUS:
        out += [f'xcd_grid {n_cu} {it} {_xcd_grid(n_cu, it)}' for it in ITEMS]
        out.append(f'xcd_grid {n_cu} uncapped {_xcd_grid_uncapped(n_cu)}')
        out += [f'cu_grid {n_cu} {t} {_cu_grid(n_cu, t)}' for t in (1, n_cu - 1, n_cu, n_cu + 1)]
    for M, N, BM, BN in ((255, 63, 256, 256), (256, 256, 256, 256), (257, 257, 256, 256), (14492, 1280, 256, 256), (1, 1, 128, 128),
                         ((2 ** 31 - 1) * 256 - 255, 256, 256, 256), (65536 * 256, 32768 * 256 - 255, 256, 256)):
        tc = _tile_counts(M, N, BM, BN)
        out.append(f'tile_counts {M} {N} {BM} {BN} ' + ('refused' if tc is None else f'ok {tc[0]} {tc[1]}'))
    out += [f'l2_nchunk bf16 {K} {_nchunk_bf16(K)}' for K in (64, 128, 256, 768, 1024, 1088, 3072)]
    out += [f'l2_nchunk mxfp8 {K} {_nchunk_mxfp8(K)}' for K in (128, 768, 2048, 2176)]
    # getenv + atoi: unset -> the default (7); "0", "12", "-3" as atoi reads them; a `static const int` initialised under "12" keeps 12 after the program has
    # set the variable to "34" (which a fresh read sees)
    out += ['env_int unset 7', 'env_int 0 0', 'env_int 12 12', 'env_int -3 -3', 'env_static 12 12 34']
    return out


def test_expectations_hold_the_cases_other_tests_rely_on():
    exp = _expected()
    assert 'l2_nchunk bf16 1024 4' in exp                                 # the tile-walk cases of tests/test_gemm_gpu.py are sized for four column tiles per sweep
    assert f'tile_counts {(2 ** 31 - 1) * 256 - 255} 256 256 256 ok 1 {2 ** 31 - 1}' in exp
    assert f'tile_counts {65536 * 256} {32768 * 256 - 255} 256 256 refused' in exp
    assert 'xcd_grid 7 1 8' in exp and 'xcd_grid 304 2147483647 304' in exp and 'xcd_grid 255 uncapped 248' in exp and 'cu_grid 1 0 0' in exp


def test_launch_plan_rules_match_the_launchers_formulas(tmp_path):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'a host C++ compiler is needed (the build needs one as well)'
    exe = tmp_path / 'launch_plan_main'
    # the header alone, with no HIP include path: it has to stand as plain C++17.  The sanitizer runtimes are linked INTO the program, so that it starts the same
    # whatever else the loader maps in front of it.
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-static-libasan', '-static-libubsan', f'-I{ROOT / "synchformer_amd" / "csrc"}', str(ROOT / 'tests' / 'launch_plan_main.cpp'), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == '', (run.returncode, run.stderr[-2000:])
    got, exp = run.stdout.splitlines(), _expected()
    assert len(got) == len(exp), (len(got), len(exp))
    for g, e in zip(got, exp):
        assert g == e, f'the header gives "{g}", the launchers computed "{e}"'
