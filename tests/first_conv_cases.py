"""The 3-channel 3x3 / pad 1 first conv (csrc/conv.h FirstGeom: VGG and DynamicCNN at stride 1, MobileNet-V2 and EfficientNet at stride 2) as
data: what the weight-gradient plan and the conv-GEMM route return for its virtual four-tap geometry, and where the plans refuse an image.

PINS: ((N, H, W), stride, element bytes) -> (the eight values of mmskin_conv_wgrad_plan, the nine of mmskin_conv_route op 3 without flags) for
a 3 -> 64 conv.  Recorded from the library of commit 4961f46, before the geometry was written once.  33 x 47: odd sizes, so the padded
width's rounding to an even number matters; 240 x 240: the largest output the weight-gradient kernels step over."""

PINS = {
    ((2, 16, 16), 1, 2): ((2, 64, 128, 0, 1, 512, 0, 8192), (0, 128, 128, 64, 2, 0, 0, 4, 1)),
    ((2, 16, 16), 1, 4): ((0, 64, 128, 0, 4, 128, 0, 32768), (0, 128, 128, 64, 2, 0, 0, 4, 1)),
    ((3, 33, 47), 1, 2): ((2, 64, 128, 0, 4, 1280, 0, 32768), (0, 128, 128, 64, 2, 0, 0, 37, 1)),
    ((3, 33, 47), 1, 4): ((0, 64, 128, 0, 30, 160, 0, 245760), (0, 128, 128, 64, 2, 0, 0, 37, 1)),
    ((2, 240, 240), 1, 2): ((0, 64, 128, 0, 450, 256, 1, 3686400), (0, 128, 128, 64, 1, 0, 0, 900, 1)),
    ((2, 240, 240), 1, 4): ((0, 64, 128, 0, 900, 128, 1, 7372800), (0, 128, 128, 64, 1, 0, 0, 900, 1)),
    ((2, 16, 16), 2, 2): ((2, 64, 128, 0, 1, 128, 0, 8192), (0, 128, 128, 64, 2, 0, 0, 1, 1)),
    ((2, 16, 16), 2, 4): ((0, 64, 128, 0, 1, 128, 0, 8192), (0, 128, 128, 64, 2, 0, 0, 1, 1)),
    ((3, 33, 47), 2, 2): ((2, 64, 128, 0, 1, 1280, 0, 8192), (0, 128, 128, 64, 2, 0, 0, 10, 1)),
    ((3, 33, 47), 2, 4): ((0, 64, 128, 0, 8, 160, 0, 65536), (0, 128, 128, 64, 2, 0, 0, 10, 1)),
    ((2, 240, 240), 2, 2): ((2, 64, 128, 0, 25, 1152, 0, 204800), (0, 128, 128, 64, 2, 0, 0, 225, 1)),
    ((2, 240, 240), 2, 4): ((0, 64, 128, 0, 225, 128, 1, 1843200), (0, 128, 128, 64, 2, 0, 0, 225, 1)),
}

# (arch, H, W, created): the weight-gradient kernels take a first-conv OUTPUT of at most 240 x 240, so the stride-1 plans stop at a
# 240 x 240 image and the stride-2 plans at 480 x 480 (481 and 482 both give 241).  Checked against the same commit's library.
DYNAMIC = "dynamic-cnn/64/l1/p0/k3"
LIMITS = [
    ("vgg16-features", 240, 240, True), ("vgg16-features", 241, 241, False), ("vgg16-features", 240, 241, False), ("vgg16-features", 241, 64, False),
    (DYNAMIC, 240, 240, True), (DYNAMIC, 241, 241, False),
    ("mobilenet-v2", 241, 241, True), ("mobilenet-v2", 480, 480, True), ("mobilenet-v2", 481, 481, False), ("mobilenet-v2", 482, 482, False),
    ("efficientnet-b0", 480, 480, True), ("efficientnet-b0", 482, 482, False),
    ("efficientnet-b7", 480, 480, True), ("efficientnet-b7", 482, 482, False),
]
