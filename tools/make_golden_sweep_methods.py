"""Generate tests/golden/sweep_wb_{linear_probing,adapter_reg}.npz from the REFERENCE's own sweep driver,
run_multiple/final_main_iteration_wb.py, for the two methods whose sweeps run on the replica-batched linear-probe and adapter
kernels.

tools/make_golden_sweep.py does the work (load_driver, main_block, run_driver, gen: the driver's unmodified seed loop and table code on
the CPU over a synthetic embedding set, every pass recorded, the runs on inputs scaled by 1 + 2^-23 and 1 + 2^-20 next to it, and the
condition that the perturbed runs select the same best epoch for every seed asserted before anything is written); this file only
holds the two configurations.  Only numbers and names are saved.

    python tools/make_golden_sweep_methods.py [linear_probing] [adapter_reg]      # default: both
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden_sweep as MS  # noqa: E402

# three seeds of the reference's default method: 1025 = 8 x 128 + 1 train rows leave a one-row last batch; step decay
LINEAR_PROBING = dict(seed=67, n_train=1025, n_val=1200, n_test=768, dim=1024,
                      argv=["--dataset", "celeba", "--tl_method", "linear_probing", "--epochs", "5", "--batch_size", "128",
                            "--learning_rate", "0.05", "--lr_decay_epochs", "3,4", "--lr_decay_rate", "0.5", "--num_iter", "3",
                            "--random_seeds", "42,32,22"])
# three seeds of adapter_reg with the per-epoch balanced reg subset and the group prompts in the reg loop
ADAPTER_REG = dict(seed=71, n_train=1024, n_val=1200, n_test=768, dim=1024,
                   argv=["--dataset", "celeba", "--tl_method", "adapter_reg", "--balance_val", "--epochs", "4", "--batch_size", "256",
                         "--batch_size_reg", "16", "--learning_rate", "0.1", "--lr_decay_epochs", "3", "--lr_decay_rate", "0.5",
                         "--num_iter", "3", "--random_seeds", "42,32,22"])
CONFIGS = {"linear_probing": LINEAR_PROBING, "adapter_reg": ADAPTER_REG}

if __name__ == "__main__":
    for name in [a for a in sys.argv[1:] if a in CONFIGS] or list(CONFIGS):
        MS.gen(CONFIGS[name], f"sweep_wb_{name}.npz")
