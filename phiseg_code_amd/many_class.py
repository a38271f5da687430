"""Which entry point of libphx serves a class count.

The kernels that meet class counts come in two families (include/phx.h, "many classes"): the narrow entries hold one pixel's classes in
registers and take 2 <= C <= 8, the wide entries of csrc/many_class.hip walk the classes in chunks and take 9 <= C <= 256.  The host
chooses by C alone, here, in pure functions: for C <= 8 every launch is the one it always was."""

MAX_NARROW_CLASSES = 8        # CE_MAXC, MC_MAXC, MT_MAXC, EV_MAXC of the narrow kernels
MAX_CLASSES = 256             # the range of the u8 label maps
MAX_ONEHOT_LABELS = 4         # the reference interpolates label maps as one-hot planes up to here (data/batch_provider.py:204, 221, 245)


def check_nlabels(nlabels, what="exp_config.nlabels"):
    """2 <= nlabels <= 256, ValueError otherwise -> int(nlabels)"""
    n = int(nlabels)
    if n != nlabels or not 2 <= n <= MAX_CLASSES:
        raise ValueError("%s must be an integer in 2 .. %d (label maps are uint8), got %r" % (what, MAX_CLASSES, nlabels))
    return n


def _wide(C):
    C = check_nlabels(C, "the class count")
    return C > MAX_NARROW_CLASSES


def residual_ce_entry(C):
    """Short name of the entry behind the residual_ce and aggregate operators."""
    return "residual_ce_wide" if _wide(C) else "residual_ce"


def xent_map_entry(C):
    """Short name of the entry behind eval_xent."""
    return "softmax_xent_map_wide" if _wide(C) else "softmax_xent_map"


def validation_metrics_entry(C):
    """Short name of the entry behind utils._metrics_device (labels [I][M][P], the Dice reference a map)."""
    return "metrics_wide" if _wide(C) else "validation_metrics"


def eval_metrics_entry(C):
    """Short name of the entry behind evaluate.evaluate_split (labels [I][P][M], the Dice reference an annotator index)."""
    return "metrics_wide" if _wide(C) else "eval_metrics"


def metrics_row(C):
    """Floats per image of the score table: GED, NCC, then the Dice slots (8 of them with the narrow entries)."""
    return 2 + max(check_nlabels(C, "the class count"), MAX_NARROW_CLASSES)


def label_route(nlabels):
    """How DeviceBatchProvider resamples label maps: "onehot" (phx_augment_batch / phx_augment_batch_elastic: one-hot planes,
    interpolated and arg-maxed) up to four labels, "nearest" (phx_augment_batch_nearest) above -- the reference's own switch."""
    return "nearest" if check_nlabels(nlabels, "nlabels") > MAX_ONEHOT_LABELS else "onehot"
