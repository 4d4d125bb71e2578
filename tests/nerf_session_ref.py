"""What one `NeRFReal.test_step` (nerfreal.py:70-127) does around `model.render`, restated in torch / numpy from the reference's lines for the NerfSession tests
(the GPU box has no reference checkout, and cv2 is not needed for two channel reversals):

    provider.py:276-283, 351      the live loader's indices: 2 * N of them, mirrored for everything but the audio
    provider.py:316-330           the torso image over the background -> bg_color, in fp32 (preload 0 / 1) or half (preload 2)
    utils.py:78-81, 1208-1212     linear_to_srgb, the resize to the GUI size
    nerfreal.py:98-122            the custom-video frame, (image * 255).astype(np.uint8), the --fullbody paste

Nothing here imports the reference or the package under test."""
import numpy as np
import torch
import torch.nn.functional as F


def mirror_index(size, index):                                   # provider.py:276-283 (= basereal.py:133-139)
    turn = index // size
    res = index % size
    if turn % 2 == 0:
        return res
    else:
        return size - res - 1


def loader_sequence(size, steps):
    """(audio index, mirrored index) of `steps` consecutive frames: `dataloader()` lists range(2 * size) (provider.py:351), test_step starts the loader again
    when it runs out (nerfreal.py:72-76), `collate` reads the audio at the original index and mirrors the rest (provider.py:292-298)."""
    out = []
    for k in range(steps):
        i = k % (2 * size)
        out.append((i, mirror_index(size, i)))
    return out


def collate_background(torso_rgba_u8, bg_img, preload):
    """provider.py:186 / 321 + 198 + 212 + 238 + 323-324: torso_rgba_u8 uint8 [H, W, 4] (numpy), bg_img fp32 [H, W, 3] (CPU tensor) -> bg_color [H * W, 3],
    fp32 for preload 0 / 1, half for preload 2 (the render casts it to fp32)."""
    t = torch.from_numpy(torso_rgba_u8.astype(np.float32) / 255)[None]
    bg = bg_img
    if preload > 1:
        t, bg = t.to(torch.half), bg.to(torch.half)
    out = t[..., :3] * t[..., 3:] + bg * (1 - t[..., 3:])
    return out.view(-1, 3)


def constant_background(name, H, W):                             # provider.py:203-206
    return torch.from_numpy(np.ones((H, W, 3), dtype=np.float32) if name == "white" else np.zeros((H, W, 3), dtype=np.float32))


def linear_to_srgb(x):                                           # utils.py:78-81
    return torch.where(x < 0.0031308, 12.92 * x, 1.055 * x ** 0.41666 - 0.055)


def gui_image(preds, H, W, color_space="srgb"):
    """utils.py:1208-1212: preds [1, h, w, 3] (any float dtype: float64 gives the exact-arithmetic yardstick) -> [H, W, 3] numpy"""
    if color_space == "linear":
        preds = linear_to_srgb(preds)
    preds = F.interpolate(preds.permute(0, 3, 1, 2), size=(H, W), mode="bilinear").permute(0, 2, 3, 1).contiguous()
    return preds[0].detach().cpu().numpy()


def to_frame(image):                                             # nerfreal.py:110
    return (image * 255).astype(np.uint8)


def bgr2rgb(image):                                              # cv2.cvtColor(image, cv2.COLOR_BGR2RGB), nerfreal.py:101, 119
    return np.ascontiguousarray(image[..., ::-1])


def fullbody_paste(image, body_bgr, start_x, start_y):
    """nerfreal.py:118-122; numpy raises ValueError when the slice leaves the body frame"""
    image_fullbody = bgr2rgb(body_bgr)
    image_fullbody[start_y:start_y + image.shape[0], start_x:start_x + image.shape[1]] = image
    return image_fullbody


def custom_frame(custom_img_cycle, custom_index, audiotype1):
    """nerfreal.py:99-102 (custom_index is advanced in place)"""
    mirindex = mirror_index(len(custom_img_cycle[audiotype1]), custom_index[audiotype1])
    image = bgr2rgb(custom_img_cycle[audiotype1][mirindex])
    custom_index[audiotype1] += 1
    return image


def is_custom(audiotype1, audiotype2, custom_index):            # nerfreal.py:98
    return audiotype1 != 0 and audiotype2 != 0 and custom_index.get(audiotype1) is not None
