"""The SP training patch set from a device-resident set: what the reference's ``ImageDataset.__getitem__`` does with its fourteen
planes (``sp_scripts_train/dataset.py:37-144``: one ``CropImg`` window, one of eight ``RotationFlip`` cases, ``ToTensor``) as one launch of
``sstem_crop_orient_f32`` (``include/sstem_batch.h``).  The four reversed masks (``255 - mask``, ``dataset.py:53-60``) are not resident
images of their own: their channels read the mask's image with the invert bit set.

    patches = sp_patches(resident, ids14, origin, case)   # ids14 [B][14], origin [B] of (row, column), case [B] of 0..7
    patches["img_2_degra"]                                  # [B,1,S,S] fp32

``if_bdadjust`` (PIL colour jitter on the two degraded sections) and ``if_use_vfiImg`` are not built.  GPU only.
"""
from data.resident import SP_ROTATION_FLIP, crop_f32, sample_table

SP_NAMES = ("img_1", "img_2", "img_2_degra", "img_3", "img_3_degra", "img_4",
            "img_2_degraB1_mask_gradall", "img_3_degraB1_mask_gradall", "img_2_degraB1_mask_gradall_r", "img_3_degraB1_mask_gradall_r",
            "img_2_degraB1_GenGradMask", "img_3_degraB1_GenGradMask", "img_2_degraB1_GenGradMask_r", "img_3_degraB1_GenGradMask_r")
SP_REVERSED = {8: 6, 9: 7, 12: 10, 13: 11}              # channel of a reversed mask -> channel of the mask it reverses
SP_INVERT = sum(1 << c for c in SP_REVERSED)


def sp_patches(resident, ids14, origin, case, patch_size, if_bdadjust=False):
    """ids14[b][c]: the resident image of plane c of sample b, in ``SP_NAMES`` order; the entries of the four reversed masks are ignored
    (``None`` will do) -- they read their mask's image.  origin[b] = (ran_h, ran_w) of ``CropImg``, case[b] the ``RotationFlip`` case.
    Returns the dataset's dict; each value is a ``[B,1,S,S]`` view of one ``[B,14,S,S]`` tensor."""
    if if_bdadjust:
        raise NotImplementedError("if_bdadjust is PIL colour jitter on the host; it is not built")
    samples, planes = [], []
    for ids, (oy, ox), a in zip(ids14, origin, case):
        if len(ids) != len(SP_NAMES):
            raise ValueError("a sample names fourteen planes")
        samples.append((oy, ox, SP_ROTATION_FLIP[a]))
        planes.append([ids[SP_REVERSED.get(c, c)] for c in range(len(SP_NAMES))])
    table = sample_table(samples, planes, resident.device)
    out, _ = crop_f32(resident, table, patch_size, patch_size, list(range(len(SP_NAMES))), len(SP_NAMES), SP_INVERT)
    return {name: out[:, c:c + 1] for c, name in enumerate(SP_NAMES)}
