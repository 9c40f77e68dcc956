"""CPU: the host side of WhittedIntegrator (src/integrators/whitted.rs) — the ABI value, the render desc the integrator name maps to, the
Python mirror of WhittedIntegrator::new, the Halton table a worst-case specular tree needs, and the Rust shim's arm for it."""
import os
import re

from rs_pbrt_amd import abi, scenes
from rs_pbrt_amd.integrator import WhittedIntegrator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_value_matches_the_header():
    src = open(os.path.join(ROOT, "include", "rspt.h")).read()
    m = re.search(r"RSPT_INTEGRATOR_WHITTED\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == abi.INTEGRATOR_WHITTED
    assert len({abi.INTEGRATOR_PATH, abi.INTEGRATOR_AO, abi.INTEGRATOR_DIRECT, abi.INTEGRATOR_VOLPATH, abi.INTEGRATOR_WHITTED}) == 5


def test_the_integrator_name_maps_to_whitted():
    rd = scenes.make_render_desc(16, 16, 4, ((0, 0, -5), (0, 0, 0), (0, 1, 0)), 40.0, integrator="whitted")
    assert rd.integrator == abi.INTEGRATOR_WHITTED   # (an unknown name still means "path")
    assert scenes.make_render_desc(16, 16, 4, ((0, 0, -5), (0, 0, 0), (0, 1, 0)), 40.0, integrator="no such").integrator == abi.INTEGRATOR_PATH


def test_python_mirror_defaults():
    rd = scenes.make_render_desc(16, 16, 4, ((0, 0, -5), (0, 0, 0), (0, 1, 0)), 40.0)
    d = WhittedIntegrator(camera=rd)._desc()
    assert d.integrator == abi.INTEGRATOR_WHITTED and d.max_depth == 5   # api.rs:246-252
    assert WhittedIntegrator(2, camera=rd)._desc().max_depth == 2


def test_halton_table_covers_the_worst_case_tree():
    """depth d, n lights: 5 camera dimensions, then per shading node 2 per light + 2 + 2 (the two sample_f draws), 2^d - 1 nodes; capped at 999"""
    primes = scenes.first_primes(1000)
    for depth in (0, 1, 3, 5, 7):
        for nl in (1, 3, 8):
            rd = scenes.make_render_desc(16, 16, 4, ((0, 0, -5), (0, 0, 0), (0, 1, 0)), 40.0, integrator="whitted", sampler="halton",
                                         max_depth=depth, light_samples=[1] * nl)
            dims = min(999, 5 + ((1 << max(depth, 1)) - 1) * (2 * nl + 4))
            assert rd.tables.n_halton_perms >= sum(primes[:dims]), (depth, nl)


def test_rust_shim_has_a_whitted_arm():
    gpu_rs = open(os.path.join(ROOT, "rust_shim", "gpu.rs")).read()
    assert "integrator without a GPU path (whitted)" not in gpu_rs
    assert "SamplerIntegrator::Whitted(" in gpu_rs
    patch = open(os.path.join(ROOT, "rust_shim", "rs_pbrt.patch")).read()
    assert "+++ b/src/integrators/whitted.rs" in patch and "fn max_depth(&self) -> u32 { self.max_depth }" in patch.split("+++ b/src/integrators/whitted.rs")[1]
