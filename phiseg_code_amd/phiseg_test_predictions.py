"""phiseg_test_predictions.py of the reference: per-label Dice of the mean prediction (100 samples; 1 for the deterministic U-Net)
of the 'best_dice' checkpoint against one randomly chosen annotation per test image, written as dice_best_dice.npz (one unnamed array
[n, nlabels]) into the experiment folder.

    python -m phiseg_code_amd.phiseg_test_predictions EXP_PATH

The reference walks the test split in shuffled order (iterate_batches); here the rows are in data-set order -- the means it logs do
not depend on the order."""
import logging
import os
import sys

import numpy as np

from phiseg_code_amd import evaluate

MODEL_SELECTION = 'best_dice'


def default_num_samples(exp_config):
    from phiseg_code_amd.phiseg.model_zoo import likelihoods
    return 1 if exp_config.likelihood is likelihoods.det_unet2D else 100


def output_file(model_path):
    return os.path.join(model_path, 'dice_%s.npz' % MODEL_SELECTION)


def main(model_path, exp_config, do_plots=False, n_samples=None, data=None):
    """do_plots is accepted for the reference's signature and ignored; n_samples (default 100, or 1 for likelihoods.det_unet2D) and
    data (default: the data set of exp_config.data_identifier) are for tests and short runs.  -> dice [n, nlabels]"""
    n_samples = default_num_samples(exp_config) if n_samples is None else int(n_samples)
    model, test = evaluate.load_model_and_test_split(model_path, exp_config, MODEL_SELECTION, data)
    logging.info('Scoring %d test images with %d samples each' % (test.images.shape[0], n_samples))
    dice_arr = evaluate.evaluate_split(model, test, n_samples)['dice']
    mean_per_lbl_dice = dice_arr.mean(axis=0)
    logging.info('Dice')
    logging.info(mean_per_lbl_dice)
    logging.info(np.mean(mean_per_lbl_dice))
    logging.info('foreground mean: %f' % (np.mean(mean_per_lbl_dice[1:])))
    np.savez(output_file(model_path), dice_arr)
    return dice_arr


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(asctime)s %(message)s')
    main(*evaluate.parse_command_line(sys.argv[1:], "Script for a simple test loop evaluating a network on the test dataset"),
         do_plots=False)
