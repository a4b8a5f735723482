/* Stand-in for the build's config.h: the block sources include it under HAVE_CONFIG_H and use nothing from it. */
