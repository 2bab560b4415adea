// Driver of tests/test_cpp_rays.py: HipIntegrator::render_rays (3dg-vol-renderer_amd/include/vr/integrator.h) on the
// main pinhole camera's own rays, next to the same integrator's frame.
//   cpp_rays SCENE W H ENV_SAMPLES OUT
// writes raw float32 to OUT: the grid's rgb (3 W H), its transmittance (W H), the frame's rgb (3 W H).
// With W = 0 nothing is rendered: only the headers and the library are exercised (CPU build check).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <numbers>
#include <vector>

#include "vr/test_integrators.h"

int main(int argc, char** argv) {
    try {
        if (argc != 6) throw std::runtime_error("usage: cpp_rays SCENE W H ENV_SAMPLES OUT");
        const uint32_t W = (uint32_t)std::atoi(argv[2]), H = (uint32_t)std::atoi(argv[3]);
        Scene scene = Scene::load_GMM(argv[1]);
        std::cout << "scene: " << scene.get_num_primitives() << " primitives\n";
        // tests/main.cpp:18-34: camera (0, 1, 6) looking at (0, 1, 0), FOV pi / 4
        const Eigen::Vector3f pos(0.0f, 1.0f, 6.0f), lookat(0.0f, 1.0f, 0.0f);
        auto cam = std::make_shared<Pinhole_Camera>(pos, (lookat - pos).normalized(), (float)(0.25 * std::numbers::pi));
        RayMarchingGaussians integ(cam, 0.01f, std::atoi(argv[4]), 0);
        std::vector<Ray> rays;
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x)
                rays.push_back(cam->sample_ray(Eigen::Vector2d(((float)x + 0.5f) / (float)W, ((float)y + 0.5f) / (float)H)));
        if (W == 0 || H == 0) return 0;
        Image grid(W, H), frame(W, H);
        std::vector<float> tr;
        integ.render_rays(scene, rays, W, H, grid, &tr);
        integ.render(scene, frame);
        FILE* f = std::fopen(argv[5], "wb");
        if (!f) throw std::runtime_error("cannot write the output file");
        std::fwrite(grid.data(), sizeof(float), 3 * (size_t)W * H, f);
        std::fwrite(tr.data(), sizeof(float), tr.size(), f);
        std::fwrite(frame.data(), sizeof(float), 3 * (size_t)W * H, f);
        std::fclose(f);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "cpp_rays: " << e.what() << "\n";
        return 1;
    }
}
