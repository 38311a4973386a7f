"""TEST INFRASTRUCTURE ONLY — the parity oracle (see rt_oracle.cpp header).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
import this.  The product (raytracing-clj_amd/) never does.
"""
from .oracle import MODE_BOOK64, MODE_MIRROR32, MODE_REF64, MODE_REALM64, MODE_REALM32, MODE_REF64D, \
    MODE_REALM64D, MODES64, DIRECT, DIRECT_SPHERE, DIRECT_DISK, build, render, features, sphere_hit, reflect, refract, \
    reflectance, quantize, camera, rng_stream, lambertian_dir, metal_dir, dielectric_dir, sampler_draws, \
    sampler_draws64, direct_from_uniforms, sampler_bias, turn24  # noqa: F401
