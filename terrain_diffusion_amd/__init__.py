"""MI355X-native InfiniteDiffusion sampling engine — Python host side over the C-ABI (include/td_engine.h).

Drop-in surface for the hot path of xandergos/terrain-diffusion: EDMUnet2D, the EDM
DPM-Solver++ scheduler, the bounded tiled samplers, the portable tile-seeded noise field and the
InfiniteTensor operator layer.  The compute runs in hand-written HIP kernels (csrc/); there is no CPU
fallback — importing is cheap, the first call that needs the engine raises if the HIP library or a GPU is missing.
"""
from ._lib import TdError, LIB_PATH, EXPORTS  # noqa: F401
from .unet import EDMUnet2D  # noqa: F401
from .autoencoder import EDMAutoencoder  # noqa: F401
from .scheduler import EDMDPMSolverMultistepScheduler  # noqa: F401
from .sampling import sample_base_diffusion, sample_base_consistency, sample_independent_tiles, _tile_starts, _linear_weight_window, _process_cond_img  # noqa: F401
from .sampling import sample_decoder_diffusion_tiled, sample_decoder_consistency_tiled, sample_coarse_tiled  # noqa: F401
from .sampling import sample_tiles_edm, score_scaling_table  # noqa: F401
from .noise import gaussian_noise_patch, gaussian_noise_patches, standard_normal, next_seed, _tile_seed  # noqa: F401
from .world_pipeline import WorldPipeline  # noqa: F401
from .infinite_tensor import InfiniteTensor, TensorWindow, MemoryTileStore, DeviceTileStore, HDF5TileStore  # noqa: F401
from .relief import relief_map, get_relief_map  # noqa: F401
from .hydrology import (flow_directions, flow_accumulation_map, flow_indicator, fill_depressions, d8_flow, flow_accumulation,  # noqa: F401
                        plot_flow_indicator, fill_depressions_priority_flood)
from .minecraft import (get_upsampled, classify_biome, get_terrain, minecraft_terrain, minecraft_payload, noise_planes,  # noqa: F401
                        parse_minecraft_payload)
from .explorer import (coarse_channels, colorize, relief_rgba8, raw_tile, land_tiles, coarse_image, coarse_stats, coarse_data,  # noqa: F401
                       detail_image, detail_raw, sample_land_tiles, get_coarse_climate_info, png_bytes)
from .rivers import relief_overlay_map, smooth_bumps, river_relief_map, smooth_river_bumps  # noqa: F401  (get_relief_map stays relief.py's)
from .custom_world import (rasterize_cells, fill_nearest, elevation_int16, h_to_meters, fill_nodata, rasterize_layer, azgaar_layers,  # noqa: F401
                           load_and_pad, import_conditioning, export_elevation)
from .dataset import (fill_voids, block_median, laplacian_encode, land_share, moments, mask_voids, prepare_chunks, prepare_and_encode,  # noqa: F401
                      RunningStats, calculate_stats_welford)
from .coarse_dataset import (area_resize_width, tile_stats, crop_scores, fill_oceans_device, fill_oceans, latitude_bands,  # noqa: F401
                             build_coarse_bands)
from .beauty import (decode_terrain, radial_spectrum, beauty_features, analyze_terrain_frequency, calculate_beauty_score, beauty_class,  # noqa: F401
                     assign_beauty_scores)
from .train_data import (DeviceGroups, views, sample_latents, cond_image, cond_vector, H5LatentsDataset, H5DecoderTerrainDataset,  # noqa: F401
                         H5AutoencoderDataset)
from .objective import (noise_levels, add_noise, logvar, squared_error, v_loss, terrain_uint8, validation_loss, noise_loss_curve)  # noqa: F401
