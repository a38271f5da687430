"""phiseg_test_quantitative.py of the reference: GED and variance-NCC of every test image over 50 samples of the 'best_ged' checkpoint,
written as ged50_best_ged.npz / ncc50_best_ged.npz (one unnamed array each) into the experiment folder.

    python -m phiseg_code_amd.phiseg_test_quantitative EXP_PATH

The samples never leave the GPU (phiseg_code_amd/evaluate.py).  As in the reference a constant NCC map gives a NaN for that image, and
the logged mean is then NaN too."""
import logging
import os
import sys

import numpy as np

from phiseg_code_amd import evaluate

N_SAMPLES = 50
MODEL_SELECTION = 'best_ged'


def output_files(model_path, n_samples=N_SAMPLES):
    """-> (GED file, NCC file)"""
    return tuple(os.path.join(model_path, '%s%d_%s.npz' % (m, n_samples, MODEL_SELECTION)) for m in ('ged', 'ncc'))


def main(model_path, exp_config, do_plots=False, n_samples=None, data=None):
    """do_plots is accepted for the reference's signature and ignored; n_samples (default 50) and data (default: the data set of
    exp_config.data_identifier) are for tests and short runs.  -> (ged [n], ncc [n])"""
    n_samples = N_SAMPLES if n_samples is None else int(n_samples)
    model, test = evaluate.load_model_and_test_split(model_path, exp_config, MODEL_SELECTION, data)
    logging.info('Scoring %d test images with %d samples each' % (test.images.shape[0], n_samples))
    res = evaluate.evaluate_split(model, test, n_samples)
    ged_arr, ncc_arr = res['ged'], res['ncc']
    for name, arr in (('GED', ged_arr), ('NCC', ncc_arr)):
        logging.info('-- %s: --' % name)
        logging.info(np.mean(arr))
        logging.info(np.std(arr))
    for path, arr in zip(output_files(model_path, n_samples), (ged_arr, ncc_arr)):
        np.savez(path, arr)
    return ged_arr, ncc_arr


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(asctime)s %(message)s')
    main(*evaluate.parse_command_line(sys.argv[1:], "Script for a simple test loop evaluating a network on the test dataset"),
         do_plots=False)
