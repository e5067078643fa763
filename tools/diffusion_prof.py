# tools/diffusion_prof.py -- the workload of profiles/diffusion_kernel_stats.csv: 3-D GLM-MHD (PPM + HLLD, VL2) with
# anisotropic conduction, viscosity and Ohmic resistivity on 8 x 128^3, six cycles through the flux-array stages.
#   rocprofv3 --kernel-trace --stats -d prof -o diff -- python tools/diffusion_prof.py
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from athenapk_amd import decks, driver
ov = ["parthenon/mesh/nx1=256", "parthenon/mesh/nx2=256", "parthenon/mesh/nx3=256",
      "parthenon/meshblock/nx1=128", "parthenon/meshblock/nx2=128", "parthenon/meshblock/nx3=128",
      "diffusion/integrator=unsplit", "diffusion/conduction=anisotropic", "diffusion/conduction_coeff=fixed",
      "diffusion/thermal_diff_coeff_code=1e-4", "diffusion/viscosity=isotropic", "diffusion/viscosity_coeff=fixed",
      "diffusion/mom_diff_coeff_code=1e-4", "diffusion/resistivity=ohmic", "diffusion/resistivity_coeff=fixed",
      "diffusion/ohm_diff_coeff_code=1e-4"]
s = driver.Simulation(decks.load("synthetic_mhd"), ov, strict=False).initialize()
assert s.info.fused == 0
for _ in range(6):
    s.step()
torch.cuda.synchronize()
print("cycles", s.ncycle, "dt", s.dt)
s.close()
