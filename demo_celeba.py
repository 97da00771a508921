"""Counterpart of reference demo_celeba.py (128x128 CelebA stack, demo_celeba.py:51-124), on the HIP kernels.
Dataset: `$DATASETS_DIR/celeba_128.npy` (float32 [N,128,128,3] in [-1,1]) when present, else synthetic batches.
`--dataset PATH` (a uint8 [N,H,W,3] .npy, e.g. CelebA at its native 218x178) trains from a device-resident `DeviceDataset` instead:
the file goes to the GPU once, every epoch is reshuffled, ranks read disjoint shards, and one launch per batch normalises, resizes
to 128x128 and (`--flip`) mirrors."""
import argparse
import os

import numpy as np
import torch

import blurred_gan_amd as blurred_gan
from blurred_gan_amd import BlurredWGANGP, DeviceDataset, GeneratorEMA, TrainingConfig, callbacks, layers, utils
from blurred_gan_amd.checkpoint import CheckpointManager


def make_dataset(batch_size, n_batches=None, seed=0):
    """demo_celeba.py:15-48 (normalise to [-1,1], resize to 128x128, shuffle); preprocessing is expected offline."""
    path = os.path.join(os.environ.get("DATASETS_DIR", "/tmp/datasets"), "celeba_128.npy")
    rng = np.random.default_rng(seed)
    if os.path.exists(path):
        x = np.load(path, mmap_mode="r")
        idx = rng.permutation(len(x))
        n = (len(x) // batch_size) if n_batches is None else n_batches
        return (torch.from_numpy(np.ascontiguousarray(x[np.sort(idx[i * batch_size:(i + 1) * batch_size])])) for i in range(n))
    return [torch.from_numpy(rng.uniform(-1, 1, size=(batch_size, 128, 128, 3)).astype(np.float32)) for _ in range(n_batches or 16)]


class DCGANGenerator(layers.SpectralSequential):
    """demo_celeba.py:51-93."""

    def __init__(self, latent_size=100, *args, upsampling="transpose", spectral_norm=False, normalization="batch", normalize_latents=False,
                 equalized_lr=False, resample_kernel=(1, 3, 3, 1), noise=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.spectral_norm, self.equalized_lr = bool(spectral_norm), bool(equalized_lr)
        if self.spectral_norm and self.equalized_lr:
            raise ValueError("equalized_lr=True together with spectral_norm=True: W / sigma cancels the run-time coefficient")
        if noise and normalization != "pixel":
            raise ValueError("noise=True needs normalization='pixel': a NoiseInjection cannot stand in a BatchNormalization stage")
        self.latent_size = latent_size
        resize = {"transpose": None, "resize": layers.UpSampling2D,
                  "filtered": lambda: layers.FilteredUpSampling2D(resample_kernel)}[upsampling]
        pixel = {"batch": False, "pixel": True}[normalization]

        def block(reshape=None):      # behind a linear layer: the reference's BatchNormalization -> LeakyReLU, or LeakyReLU -> PixelNormalization
            if pixel and reshape:
                self.add(layers.Reshape(reshape))
            elif noise:                 # StyleGAN's per-pixel noise input, behind every hidden (transposed) convolution
                self.add(layers.NoiseInjection())
            if not pixel:
                self.add(layers.BatchNormalization())
            self.add(layers.LeakyReLU())
            if pixel:
                self.add(layers.PixelNormalization())
            elif reshape:
                self.add(layers.Reshape(reshape))
        first = dict(input_shape=(self.latent_size,))
        if normalize_latents:
            self.add(layers.PixelNormalization(**first))
            first = {}
        self.add(layers.Dense(4 * 4 * 512, use_bias=pixel, **first))
        block(reshape=(4, 4, 512))
        assert self.output_shape == (None, 4, 4, 512)
        hw = 4
        for filters, stride in ((512, 1), (256, 2), (128, 2), (64, 2), (32, 2), (16, 2)):
            if resize and stride == 2:      # resize-convolution: nearest-neighbour upsampling, then a stride-1 convolution
                self.add(resize())
                self.add(layers.Conv2D(filters, (5, 5), strides=(1, 1), padding='same', use_bias=pixel))
            else:
                self.add(layers.Conv2DTranspose(filters, (5, 5), strides=(stride, stride), padding='same', use_bias=pixel))
            hw *= stride
            assert self.output_shape == (None, hw, hw, filters), self.output_shape
            block()
        self.add(layers.Conv2D(3, (5, 5), padding='same', use_bias=False, activation='tanh'))
        assert self.output_shape == (None, 128, 128, 3), self.output_shape


class DCGANDiscriminator(layers.SpectralSequential):
    """demo_celeba.py:96-124."""

    def __init__(self, *args, downsampling="stride", normalization="none", spectral_norm=False, minibatch_stddev=0, equalized_lr=False,
                 resample_kernel=(1, 3, 3, 1), **kwargs):
        super().__init__(*args, **kwargs)
        self.spectral_norm, self.equalized_lr = bool(spectral_norm), bool(equalized_lr)
        if self.spectral_norm and self.equalized_lr:
            raise ValueError("equalized_lr=True together with spectral_norm=True: W / sigma cancels the run-time coefficient")
        pool = {"stride": None, "pool": layers.AveragePooling2D,
                "filtered": lambda: layers.FilteredDownSampling2D(resample_kernel)}[downsampling]
        norm = {"none": False, "layer": True}[normalization]
        for i, c in enumerate((16, 32, 64, 128, 256, 512)):
            kw = dict(input_shape=[128, 128, 3]) if i == 0 else {}
            self.add(layers.Conv2D(c, 5, strides=1 if pool else 2, padding='same', **kw))
            if norm:
                self.add(layers.LayerNormalization())
            self.add(layers.LeakyReLU())
            self.add(layers.Dropout(0.3))
            if pool:
                self.add(pool())
        if minibatch_stddev:
            self.add(layers.MinibatchStdDev(group_size=minibatch_stddev))
        self.add(layers.Flatten())
        self.add(layers.Dense(1, activation="linear"), gain=1.0)


def make_parser():
    """The demo's command line."""
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    BlurredWGANGP.HyperParameters.add_arguments(parser)
    TrainingConfig.add_arguments(parser)
    parser.add_argument("--epochs", type=int, default=10)
    parser.add_argument("--max_batches", type=int, default=None)
    parser.add_argument("--results_dir", default="results")
    parser.add_argument("--conv-math", dest="conv_math", default="fp32", choices=["fp32", "bf16x6"],
                        help="conv forward / data-gradient math: fp32 (default) or the opt-in split-bf16 kernels")
    parser.add_argument("--upsampling", default="transpose", choices=["transpose", "resize", "filtered"],
                        help="generator resolution steps: stride-2 Conv2DTranspose (default, the reference's), nearest-neighbour "
                             "UpSampling2D + stride-1 Conv2D (4x the multiply-adds of the layers it replaces), or the same with the "
                             "FIR-filtered FilteredUpSampling2D (StyleGAN2's upsample_2d, --resample-kernel)")
    parser.add_argument("--downsampling", default="stride", choices=["stride", "pool", "filtered"],
                        help="critic resolution steps: stride-2 Conv2D (default, the reference's), stride-1 Conv2D + AveragePooling2D "
                             "(4x the multiply-adds of the layers it replaces), or the same with the FIR-filtered "
                             "FilteredDownSampling2D (StyleGAN2's downsample_2d, --resample-kernel)")
    parser.add_argument("--resample-kernel", dest="resample_kernel", default=(1.0, 3.0, 3.0, 1.0), metavar="K",
                        type=lambda s: tuple(float(v) for v in s.split(",")),
                        help="the 1-D kernel of --upsampling filtered / --downsampling filtered: comma-separated, an even count up to 8")
    parser.add_argument("--critic-norm", dest="critic_norm", default="none", choices=["none", "layer"],
                        help="critic normalisation: none (default, the reference's) or a LayerNormalization over the channels between "
                             "every Conv2D and its LeakyReLU (the WGAN-GP paper's critic)")
    parser.add_argument("--critic-spectral-norm", dest="critic_spectral_norm", action="store_true",
                        help="spectral normalisation (Miyato et al. 2018) of every Conv2D and Dense of the critic: the step computes "
                             "with W / sigma, one power round per critic step")
    parser.add_argument("--critic-mbstd", dest="critic_mbstd", type=int, default=0, metavar="G",
                        help="minibatch standard deviation layer in front of the critic's head, over groups of G consecutive samples "
                             "(0: off; the batch size must be a multiple of G)")
    parser.add_argument("--generator-norm", dest="generator_norm", default="batch", choices=["batch", "pixel", "style"],
                        help="generator normalisation: BatchNormalization in front of every LeakyReLU (default, the reference's) or a "
                             "PixelNormalization behind it (ProGAN / StyleGAN: per pixel, no variables, no batch statistics; the Dense "
                             "and the hidden convolutions then carry a bias), or 'style': StyleGAN2's modulated convolutions with weight "
                             "demodulation, the styles taken from the latents or from --mapping-layers")
    parser.add_argument("--normalize-latents", dest="normalize_latents", action="store_true",
                        help="a PixelNormalization of the latent vectors in front of the generator's Dense")
    parser.add_argument("--generator-noise", dest="generator_noise", action="store_true",
                        help="StyleGAN's per-pixel noise inputs: a NoiseInjection (strength * N(0, 1) per pixel, one learned strength per "
                             "layer, initialised to zero) behind every hidden convolution of the generator (needs --generator-norm pixel or style)")
    parser.add_argument("--mapping-layers", dest="mapping_layers", type=int, default=0, metavar="N",
                        help="StyleGAN's mapping network in front of the generator: N Dense + LeakyReLU layers z -> w, w the style "
                             "source of the modulated convolutions (0: off; needs --generator-norm style)")
    parser.add_argument("--mapping-units", dest="mapping_units", type=int, default=None, metavar="U",
                        help="width of the mapping network and of w (default: the latent size)")
    parser.add_argument("--mapping-lr-multiplier", dest="mapping_lr_multiplier", type=float, default=0.01, metavar="M",
                        help="learning-rate multiplier of the mapping network (with --generator-equalized-lr; without it, it must be 1)")
    parser.add_argument("--truncation-psi", dest="truncation_psi", type=float, default=None, metavar="P",
                        help="the truncation trick of the sample grids: w <- w_avg + P * (w - w_avg) (needs --mapping-layers)")
    parser.add_argument("--latent-distribution", dest="latent_distribution", default="uniform", choices=["uniform", "normal"],
                        help="the latents' distribution: uniform on [0, 1) (default, the reference's) or N(0, I) (the ProGAN / StyleGAN "
                             "papers'; what --normalize-latents is meant to normalise)")
    parser.add_argument("--generator-spectral-norm", dest="generator_spectral_norm", action="store_true",
                        help="spectral normalisation of every Dense, Conv2DTranspose and Conv2D of the generator (not together with "
                             "the generator average)")
    parser.add_argument("--critic-equalized-lr", dest="critic_equalized_lr", action="store_true",
                        help="equalised learning rate (Karras et al. 2018) on every Conv2D and Dense of the critic: kernels drawn "
                             "from N(0, 1), the step computes with gain / sqrt(fan_in) * W (not together with its spectral norm)")
    parser.add_argument("--generator-equalized-lr", dest="generator_equalized_lr", action="store_true",
                        help="equalised learning rate on every Dense, Conv2DTranspose and Conv2D of the generator (not together with "
                             "its spectral norm)")
    parser.add_argument("--dataset", default=None, metavar="PATH",
                        help="uint8 .npy of images: train from a device-resident DeviceDataset (default: the data path described above)")
    parser.add_argument("--flip", action="store_true", help="with --dataset: mirror each sample left-right with probability 1/2")
    ema_group = parser.add_mutually_exclusive_group()
    ema_group.add_argument("--g-ema-decay", dest="g_ema_decay", type=float, default=None,
                           help="average the generator's weights with this decay per generator update (off by default)")
    ema_group.add_argument("--g-ema-halflife-images", dest="g_ema_halflife_images", type=float, default=None,
                           help="average the generator's weights with a half-life of this many images (off by default)")
    parser.add_argument("--diffaugment", default=None, metavar="POLICY",
                        help="differentiable augmentation of every batch the critic sees: comma-separated names out of "
                             "color, translation, cutout (off by default)")
    blurred_gan.diffaugment.add_ada_arguments(parser)
    parser.add_argument("--loss", default="wasserstein", choices=["wasserstein", "hinge", "nonsaturating"],
                        help="the pair of critic and generator losses: wasserstein (default, the reference's), hinge or the "
                             "non-saturating logistic loss")
    parser.add_argument("--penalty-on", dest="penalty_on", default="interpolates", choices=["interpolates", "reals", "fakes"],
                        help="where the critic's input gradient is penalised: the interpolates of reals and fakes (default, the "
                             "reference's), the reals (with --penalty-target 0: R1) or the fakes (R2)")
    parser.add_argument("--penalty-target", dest="penalty_target", type=float, default=1.0,
                        help="the gradient norm the penalty pulls towards: gp_coefficient * mean((norm - target)^2)")
    parser.add_argument("--penalty-interval", dest="penalty_interval", type=int, default=1, metavar="K",
                        help="lazy regularisation: the penalty runs on every K-th critic step with K times the coefficient")
    parser.add_argument("--swd-every-n-examples", dest="swd_every_n_examples", type=int, default=0, metavar="N",
                        help="measure the sliced Wasserstein distance between reals and fakes every N training examples on the "
                             "library's SWD kernels (0: off; the reference demo measures every 50000)")
    parser.add_argument("--swd-samples", dest="swd_samples", type=int, default=1000,
                        help="images per set of one SWD measurement")
    return parser


def main(argv=None):
    """demo_celeba.py:127-246; multi-GPU decisions as in demo_mnist.main (global batch = per-GPU batch x replicas, one run
    directory made by rank 0, file-writing callbacks on rank 0 only)."""
    blurred_gan.set_seed(123123)
    parser = make_parser()
    args = parser.parse_args(argv)
    hyperparameters = BlurredWGANGP.HyperParameters.from_args(args)
    config = TrainingConfig.from_args(args)
    dist = blurred_gan.dist
    num_gpus = dist.init_from_env()
    rank0 = dist.rank() == 0
    if rank0:
        print("Num gpus:", num_gpus)
    hyperparameters.global_batch_size = hyperparameters.batch_size * num_gpus
    if args.dataset:
        # sharded by rank, reshuffled every epoch; the ring buffers keep their addresses, so the step programs read them in place
        dataset = DeviceDataset(args.dataset, image_size=(128, 128), batch_size=hyperparameters.batch_size, flip=args.flip, seed=123123)
        total_n_examples = dataset.samples_per_epoch
    else:
        dataset = make_dataset(hyperparameters.batch_size, n_batches=args.max_batches, seed=dist.rank())
        total_n_examples = 202_599
    config.log_dir = dist.broadcast_object(utils.create_result_subdir(args.results_dir, "celeba") if rank0 else None)
    config.checkpoint_dir = config.log_dir + "/checkpoints"
    if args.mapping_layers and args.generator_norm != "style":
        parser.error("--mapping-layers needs --generator-norm style")
    if args.truncation_psi is not None and not args.mapping_layers:
        parser.error("--truncation-psi needs --mapping-layers")
    gen_kw = dict(upsampling=args.upsampling, spectral_norm=args.generator_spectral_norm, normalization=args.generator_norm,
                  normalize_latents=args.normalize_latents, equalized_lr=args.generator_equalized_lr,
                  resample_kernel=args.resample_kernel, noise=args.generator_noise)
    if args.generator_norm == "style":      # the modulated stack (and its mapping network) is the library's: models.DCGANGenerator
        gen = blurred_gan.models.DCGANGenerator(arch="celeba128", mapping_layers=args.mapping_layers, mapping_units=args.mapping_units,
                                                mapping_lr_multiplier=args.mapping_lr_multiplier, **gen_kw)
    else:
        gen = DCGANGenerator(**gen_kw)
    disc = DCGANDiscriminator(downsampling=args.downsampling, normalization=args.critic_norm, spectral_norm=args.critic_spectral_norm,
                              minibatch_stddev=args.critic_mbstd, equalized_lr=args.critic_equalized_lr, resample_kernel=args.resample_kernel)
    generator_ema = None
    if args.g_ema_decay is not None:
        generator_ema = GeneratorEMA(decay=args.g_ema_decay)
    elif args.g_ema_halflife_images is not None:
        generator_ema = GeneratorEMA(halflife_images=args.g_ema_halflife_images)
    gan = blurred_gan.BlurredWGANGP(gen, disc, hyperparams=hyperparameters, config=config, conv_math=args.conv_math,
                                    generator_ema=generator_ema, persistent_input=bool(args.dataset), augment=blurred_gan.diffaugment.augment_from_args(args),
                                    latent_distribution=args.latent_distribution,
                                    objective=blurred_gan.Objective(args.loss, args.penalty_target, args.penalty_on, args.penalty_interval))
    manager = CheckpointManager(gan, directory=config.checkpoint_dir, max_to_keep=5)
    if manager.latest_checkpoint:
        manager.restore(manager.latest_checkpoint)
    cbs = [callbacks.BlurDecayController(total_n_training_examples=total_n_examples * args.epochs, max_value=5)]
    if rank0:
        gan.hparams.save_json(os.path.join(config.log_dir, "hyper_parameters.json"))
        gan.config.save_json(os.path.join(config.log_dir, "train_config.json"))
        cbs = [callbacks.GenerateSampleGridCallback(log_dir=config.log_dir, every_n_examples=5_000, truncation_psi=args.truncation_psi), *cbs,
               callbacks.SaveModelCallback(manager, n=10_000), callbacks.LogMetricsCallback()]
        if args.swd_every_n_examples > 0:        # the reference's SWDMetricCallback, fed from model.images with no host work
            cbs.append(callbacks.SWDMetricCallback(None, num_samples=args.swd_samples, every_n_examples=args.swd_every_n_examples,
                                                   native=True, seed=123123))
    try:
        initial_epoch = gan.n_img // total_n_examples
        if args.dataset:
            dataset.epoch = int(initial_epoch)          # a resumed run goes on with the epoch's own order
        gan.fit(x=dataset, y=None, epochs=args.epochs, initial_epoch=initial_epoch, callbacks=cbs,
                steps_per_epoch=args.max_batches if args.dataset else None)
    except KeyboardInterrupt:
        if rank0:
            manager.save()
    dist.barrier()
    if rank0:
        print("Done training.")
    return gan


if __name__ == "__main__":
    main()
    blurred_gan.dist.shutdown()
