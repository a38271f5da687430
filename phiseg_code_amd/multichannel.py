"""Which entry point of libphx serves an image channel count Cx = exp_config.image_size[2].

The kernels that meet the image as an array of pixels come in two families (include/phx.h, "multi-channel images"): the entries that
were always there take one channel, the entries of csrc/multichannel.hip take 2 <= Cx <= 16 and refuse 1.  The host chooses by Cx
alone, here, in pure functions: for Cx = 1 every launch is the one it always was.  The cap of 16 is a choice (RGB(A) and every
multi-sequence MR protocol fit), not a measurement."""

MAX_IMAGE_CHANNELS = 16


def check_channels(Cx, what="exp_config.image_size[2]"):
    """1 <= Cx <= 16, ValueError otherwise -> int(Cx)"""
    n = int(Cx)
    if n != Cx or not 1 <= n <= MAX_IMAGE_CHANNELS:
        raise ValueError("%s must be an integer in 1 .. %d (the number of image channels), got %r" % (what, MAX_IMAGE_CHANNELS, Cx))
    return n


def check_image_size(image_size):
    """exp_config.image_size = (H, W, Cx) -> Cx, checked"""
    if len(image_size) != 3:
        raise ValueError("exp_config.image_size must be (H, W, channels) with 1 .. %d channels, got %r" % (MAX_IMAGE_CHANNELS, tuple(image_size)))
    return check_channels(image_size[2])


def posterior_input_entry(Cx):
    """Short name of the entry behind concat[x, one_hot(s) - 0.5]."""
    return "posterior_input_mc" if check_channels(Cx, "the channel count") > 1 else "posterior_input"


def augment_entry(Cx, nlabels=2, elastic=False):
    """Short name of the entry behind DeviceBatchProvider.next_batch_device: ONE entry for Cx > 1, the three single-channel entries
    (by label route and elastic stage) for Cx = 1."""
    from phiseg_code_amd import many_class
    if check_channels(Cx, "the channel count") > 1:
        many_class.check_nlabels(nlabels, "nlabels")
        return "augment_batch_mc"
    if many_class.label_route(nlabels) == "nearest":
        return "augment_batch_nearest"
    return "augment_batch_elastic" if elastic else "augment_batch"


def summary_channels(Cx):
    """Channels of the x_inp / generated_x_in image summaries: 3 or 4 image channels give a colour grid (PNG colour types 2 / 6,
    colourspace 3 / 4); any other Cx > 1 shows channel 0 in grey (tf.summary.image would refuse such a tensor; a summary must not stop
    a training run).  -> Cout"""
    return Cx if check_channels(Cx, "the channel count") in (1, 3, 4) else 1


def summary_grid_entry(Cx):
    """Short name of the entry behind the x_inp / generated_x_in grids."""
    return "summary_grid_image_mc" if check_channels(Cx, "the channel count") > 1 else "summary_grid_u8"
